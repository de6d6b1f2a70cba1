"""Brute-force index on the GPU (rbq_bf_search_batch) against the numpy restatement of BruteForceRabitqIndex::search_internal
(tests/bf_ref.py): identical ids and counts, bit-identical scores, unused slots NaN / UINT64_MAX, over bit widths, metrics,
rotators, dimensions, sizes, top_k, batch sizes, filters, duplicate vectors (the heap's tie path), non-finite queries, the
error order, threads on one handle, and RBF1 save / load."""
import ctypes as C
import threading

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import bruteforce as bfm
from rbf1_writer import write_rbf1
import bf_ref

pytestmark = pytest.mark.gpu
U64MAX = np.iinfo(np.uint64).max


def make(n, dim, bits, metric, rotator, seed, dup=0):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    if dup and n > 1:  # copies of earlier vectors: equal distances in every query
        src = rng.integers(0, max(1, n // 4), dup)
        dst = rng.integers(n // 4, n, dup)
        data[dst] = data[src]
    built = rq.builder.train_bruteforce(data, bits, metric, rotator, seed, True)
    return data, built, rq.BruteForceRabitqIndex.from_built(built), bf_ref.Prepared(built.hdr_ptr, built.arrays())


def check(idx, prep, queries, k, allowed=None, words=None, nbits=0, sample=None):
    ids, scores, counts = idx.batch_search_raw(queries, rq.BruteForceSearchParams(k), words, nbits)
    rows = range(len(queries)) if sample is None else sample
    for i in rows:
        rid, rsc = bf_ref.search(prep, queries[i], k, allowed)
        c = len(rid)
        assert counts[i] == c, (i, counts[i], c)
        assert np.array_equal(ids[i, :c], rid), (i, ids[i, :c][:10], rid[:10])
        assert np.array_equal(scores[i, :c].view(np.uint32), rsc.view(np.uint32)), i
        assert np.all(ids[i, c:] == U64MAX) and np.all(np.isnan(scores[i, c:]))
    return ids, scores, counts


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("rotator,dim", [(1, 128), (0, 32), (1, 960)])
def test_parity_bits_metric_rotator(bits, metric, rotator, dim):
    data, built, idx, prep = make(700, dim, bits, metric, rotator, 10 * bits + metric + dim)
    q = np.random.default_rng(dim).standard_normal((7, dim)).astype(np.float32)
    check(idx, prep, q, 10)
    check(idx, prep, q[:1], 100)


@pytest.mark.parametrize("n,k", [(1, 10), (5, 10), (300, 1000), (2000, 16384), (50000, 10), (3000, 1)])
def test_sizes_and_top_k(n, k):
    data, built, idx, prep = make(n, 64, 7, 0, 1, n + k)
    q = np.random.default_rng(n).standard_normal((3, 64)).astype(np.float32)
    check(idx, prep, q, k)


def test_dim_1024_and_batches():
    data, built, idx, prep = make(3000, 1024, 7, 0, 1, 77)
    rng = np.random.default_rng(1)
    for nq in (1, 64, 1500):
        q = rng.standard_normal((nq, 1024)).astype(np.float32)
        check(idx, prep, q, 10, sample=sorted(set(rng.integers(0, nq, 6).tolist()) | {0, nq - 1}))


@pytest.mark.parametrize("metric", [0, 1])
def test_duplicates_take_the_tie_path(metric):
    data, built, idx, prep = make(4000, 64, 3, metric, 1, 91 + metric, dup=1500)
    before = idx.heap_stats()
    q = np.concatenate([data[:20], np.random.default_rng(2).standard_normal((20, 64)).astype(np.float32)])
    for k in (1, 10, 100):
        check(idx, prep, q, k)
    after = idx.heap_stats()
    assert after["pushes"] > before["pushes"] and after["tie_pushes"] > before["tie_pushes"], (before, after)


def test_queries_equal_to_data_vectors_recover_them():
    """brute_force_search_recovers_identical_vectors, with our own seeds: each data vector finds itself first"""
    data, built, idx, prep = make(500, 128, 7, 0, 1, 4242)
    ids, scores, counts = check(idx, prep, data[:16], 5)
    assert np.array_equal(ids[:, 0], np.arange(16, dtype=np.uint64))


@pytest.mark.parametrize("metric", [0, 1])
def test_filters(metric):
    data, built, idx, prep = make(1200, 64, 7, metric, 1, 5 + metric)
    n = 1200
    q = np.random.default_rng(9).standard_normal((4, 64)).astype(np.float32)
    rng = np.random.default_rng(3)
    for allowed_ids in ([], list(range(n)), sorted(set(rng.integers(0, n, 300).tolist())), list(range(0, 700, 3))):
        mask = np.zeros(n, bool)
        mask[allowed_ids] = True
        words, nbits = bfm._filter_words(allowed_ids)
        check(idx, prep, q, 20, mask, words, nbits)  # (filter_nbits < n for the last two sets)
        res = idx.search_filtered(q[0], rq.BruteForceSearchParams(20), allowed_ids)
        assert all(r.id in set(allowed_ids) for r in res)


def test_non_finite_query_returns_nothing():
    data, built, idx, prep = make(300, 64, 7, 0, 1, 8)
    for bad in (np.inf, np.nan, -np.inf):
        q = np.random.default_rng(1).standard_normal((2, 64)).astype(np.float32)
        q[0, 5] = bad
        ids, scores, counts = check(idx, prep, q, 10)
        assert counts[0] == 0 and counts[1] == 10


def test_errors_in_the_crates_order_and_top_k_zero():
    data, built, idx, prep = make(50, 64, 7, 0, 1, 3)
    with pytest.raises(rq.RabitqError) as e:
        idx.search(np.zeros(10, np.float32), rq.BruteForceSearchParams(5))
    assert e.value.kind == "DimensionMismatch" and "expected 64, got 10" in str(e.value)
    assert idx.search(data[0], rq.BruteForceSearchParams(0)) == []
    with pytest.raises(rq.RabitqError) as e:
        idx.search(data[0], rq.BruteForceSearchParams(16385))
    assert e.value.kind == "InvalidConfig" and "16384" in str(e.value)
    # a loaded vector_count = 0 stream: EmptyIndex before DimensionMismatch
    h = built.header
    empty = write_rbf1(h.dim, h.padded_dim, 0, 1, 6, built.rotator_blob(), np.zeros((0, 8), np.uint8), np.zeros((0, 48), np.uint8),
                       {f: np.zeros(0, np.float32) for f in rq._abi.BF_FACTORS})
    e_idx = rq.BruteForceRabitqIndex.load_from_bytes(empty)
    assert len(e_idx) == 0 and e_idx.is_empty()
    with pytest.raises(rq.RabitqError) as e:
        e_idx.search(np.zeros(10, np.float32), rq.BruteForceSearchParams(5))
    assert e.value.kind == "EmptyIndex"


def test_two_threads_on_one_handle():
    data, built, idx, prep = make(5000, 128, 7, 1, 1, 12)
    rng = np.random.default_rng(4)
    qs = [rng.standard_normal((200, 128)).astype(np.float32) for _ in range(4)]
    serial = [idx.batch_search_raw(q, rq.BruteForceSearchParams(10)) for q in qs]
    out = [None] * 4

    def run(i):
        out[i] = idx.batch_search_raw(qs[i], rq.BruteForceSearchParams(10))
    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for a, b in zip(serial, out):
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("bits,rotator,dim", [(7, 1, 64), (3, 0, 32), (1, 1, 128)])
def test_rbf1_save_load(bits, rotator, dim, tmp_path):
    data, built, idx, prep = make(400, dim, bits, 1, rotator, 31 + bits)
    blob = idx.save_to_bytes()
    h, a = built.header, built.arrays()
    assert blob == write_rbf1(h.dim, h.padded_dim, h.metric, h.rotator, h.ex_bits, built.rotator_blob(), a["bin"], a["ex"], a)
    q = np.random.default_rng(0).standard_normal((9, dim)).astype(np.float32)
    want = idx.batch_search_raw(q, rq.BruteForceSearchParams(25))
    if bits == 1:  # the crate's 1-bit quirk: its own writer's stream does not load
        with pytest.raises(rq.RabitqError, match="checksum mismatch"):
            rq.BruteForceRabitqIndex.load_from_bytes(blob)
        blob = write_rbf1(h.dim, h.padded_dim, h.metric, h.rotator, 0, built.rotator_blob(), a["bin"], np.zeros((400, 0), np.uint8), a)
    path = tmp_path / "x.rbf"
    path.write_bytes(blob)
    loaded = rq.BruteForceRabitqIndex.load_from_path(str(path))
    assert len(loaded) == 400 and loaded.dim == dim and loaded.save_to_bytes() == blob
    got = loaded.batch_search_raw(q, rq.BruteForceSearchParams(25))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(want, got))
    assert [r.id for r in loaded.batch_search(q, rq.BruteForceSearchParams(3))[2]] == [int(i) for i in want[0][2, :3]]


def test_train_classmethod_and_search():
    data = np.random.default_rng(6).standard_normal((100, 64)).astype(np.float32)
    idx = rq.BruteForceRabitqIndex.train(data, 7, rq.Metric.L2, rq.RotatorType.FhtKacRotator, 6, True)
    res = idx.search(data[3], rq.BruteForceSearchParams(3))
    assert res[0].id == 3 and len(res) == 3 and isinstance(res[0], rq.BruteForceSearchResult)
