"""The exact brute-force top-k (rbq_bf_search_exact_batch: k_bf_dist -> k_bf_select at top_k := pool -> k_bf_rerank_score ->
k_bf_rerank_order) against its restatement (tests/bf_rerank_ref.py), every comparison exact: ids, score bits,
counts and the unused slots of every row.  Seeded.  (The scorer's accumulators start at +0.0, so a zero dot product is +0.0 and its
distance -0.0 on every row: no mixed -0.0 / +0.0 pair can arise; the zero-dot ties pin that such distances fall back to the id.)"""
import functools

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, bruteforce as bfm
import bf_range_exact_ref as xref
import bf_ref
import bf_rerank_ref as ref

pytestmark = pytest.mark.gpu
POOLS = (None, 100, 129, 4096)  # top_k itself; no power of two; one entry past the score kernel's slice of 128; the largest
# dims: scalar tail only; either side of a 128-byte span (f32 31 / 33, 16-bit 63 / 65; odd 16-bit rows go element by element);
# an even 16-bit dim past one span; 960.  1100 vectors: a pool of 4096 stays short and its last slices are empty.
DIMS = {"f32": (1, 31, 33, 960), "f16": (1, 63, 65, 72, 960), "bf16": (63, 65, 72, 960)}
KEYS = [(1100, d, (7, 1)[(i + m) % 2], m, raw) for raw in DIMS for i, d in enumerate(DIMS[raw]) for m in (0, 1)] + \
       [(4500, 20, 7, i % 2, raw) for i, raw in enumerate(DIMS)]  # a full pool of 4096: 32 slices, the order kernel's widest sort
KEY = (1100, 20, 7, 0, "f16")


@functools.lru_cache(maxsize=None)
def case(n, dim, bits, metric, nq=7):
    """(index, prep, queries near data rows, data, the builder's result: prep rotates queries with its header, so it stays alive)"""
    rng = np.random.default_rng(1000 * bits + 10 * metric + dim)
    data = (rng.standard_normal((n, dim)) + 1.0).astype(np.float32)
    q = (data[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    built = rq.builder.train_bruteforce(data, bits, metric, 1, 7, True)
    return rq.BruteForceRabitqIndex.from_built(built), bf_ref.Prepared(built.hdr_ptr, built.arrays()), q, data, built


def attached(key, rows=None):
    """(the case's index with `rows` (None: its data) attached in key's element type, prep, queries, the rows the scorer sees)"""
    idx, prep, q, data = case(*key[:4], *key[5:])[:4]
    stored, dtype, wide = xref.stored_rows(data if rows is None else rows, key[4])
    idx.set_rerank_vectors(stored, dtype=dtype)
    return idx, prep, q, wide


def run(idx, q, k, pool, chunk=0, words=None, nbits=0):
    """(ids, score bits, counts) with at most `chunk` vectors per chunk (0: no limit), and the k_bf_select launches of the call"""
    L = bfm.lib()
    assert L.rbq_bf_debug_set_chunk_vectors(chunk) == 0
    try:
        l0 = L.rbq_bf_debug_select_launches()
        ids, sc, cnt = idx.batch_search_exact_raw(q, rq.BruteForceSearchParams(k), pool, words, nbits)
        return (ids, sc.view(np.uint32), cnt), L.rbq_bf_debug_select_launches() - l0
    finally:
        L.rbq_bf_debug_set_chunk_vectors(0)


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_parity(key):
    idx, prep, q, wide = attached(key)
    for pool in POOLS:
        want, pcount = ref.rows(prep, q, wide, 10, pool)
        assert (pcount == min(key[0], pool or 10)).all() and (want[2] == 10).all()
        assert same(run(idx, q, 10, pool)[0], want), pool


@pytest.mark.parametrize("left", [6, 0])
def test_filter_leaves_fewer_than_top_k(left):
    idx, prep, q, wide = attached(KEY)
    allowed = np.zeros(KEY[0], bool)
    allowed[np.random.default_rng(5).choice(900, left, replace=False)] = True
    words, nbits = bfm._filter_words(np.nonzero(allowed)[0])
    want = ref.rows(prep, q, wide, 10, 100, allowed)[0]
    assert (want[2] == left).all() and (want[0][:, left:] == ref.U64MAX).all() and (want[1][:, left:] == ref.NAN_BITS).all()
    assert same(run(idx, q, 10, 100, 0, words, nbits)[0], want)


@pytest.mark.parametrize("metric", [0, 1])
def test_exact_ties_come_out_by_id_and_a_non_finite_entry_is_dropped(metric):
    """copies of one row, zero rows (inner product: -0.0 distances) and a row with an inf among query 0's pool; top_k = pool = 100"""
    key = (1100, 20, 7, metric, "f32")
    prep, q, data = case(*key[:4])[1:4]
    pool0 = bf_ref.search(prep, q[0], 100)[0].astype(np.int64)
    rows, dup, zero = data.copy(), np.sort(pool0[[3, 9, 4, 20]]), np.sort(pool0[[30, 31, 32]])
    rows[dup] = data[dup[0]]
    if metric == 1:
        rows[zero] = 0.0
    rows[pool0[50], 1] = np.inf
    idx, prep, q, wide = attached(key, rows)
    want = ref.rows(prep, q, wide, 100, 100)[0]
    ids0, bits0 = want[0][0].astype(np.int64), want[1][0]
    for tied in (dup, zero) if metric == 1 else (dup,):
        at = np.nonzero(np.isin(ids0, tied))[0]
        assert np.array_equal(ids0[at], tied) and (np.diff(at) == 1).all() and len(set(bits0[at])) == 1  # one run, ids ascending
    assert want[2][0] == 99 and pool0[50] not in ids0 and (metric == 0 or (bits0[np.isin(ids0, zero)] == 0).all())
    assert same(run(idx, q, 100, 100)[0], want)


def test_pool_across_three_chunks_and_a_second_sub_batch():
    idx, prep, q, wide = attached(KEY)
    got, launches = run(idx, q, 10, 100, chunk=400)  # chunks of 400, 400 and 300 vectors
    assert launches == 3 and same(got, ref.rows(prep, q, wide, 10, 100)[0])
    key = (300, 7, 7, 0, "bf16", 1025)               # 1025 queries: the plan's sub-batch is 1024
    idx, prep, q, wide = attached(key)
    got, launches = run(idx, q, 10, 20)
    assert launches == 2 and same(got, ref.rows(prep, q, wide, 10, 20)[0])


def test_other_calls_untouched_the_same_bytes_twice_and_the_python_layer():
    idx, prep, q, wide = attached(KEY)
    p = rq.BruteForceSearchParams(10)
    before = idx.batch_search_raw(q, p)
    got = run(idx, q, 10, 129)[0]
    assert same(got, ref.rows(prep, q, wide, 10, 129)[0]) and same(run(idx, q, 10, 129)[0], got)
    assert same(idx.batch_search_raw(q, p), before)
    res = idx.batch_search_exact(q, p, pool=129)
    assert [[r.id for r in row] for row in res] == got[0].tolist() and res[0] == idx.search_exact(q[0], p, pool=129)
    assert sorted(r.id for r in idx.search_exact(q[0], p, 129, allowed_ids=[5, 3])) == [3, 5]


def test_without_raw_vectors_the_call_is_refused():
    q, data = case(*KEY[:4])[2:4]
    idx = rq.BruteForceRabitqIndex.train(data, KEY[2], KEY[3], 1, 7, True)
    idx.set_rerank_vectors(data)
    idx.batch_search_exact_raw(q, rq.BruteForceSearchParams(10))
    for detach in (lambda: idx.set_rerank_vectors(None), lambda: (idx.set_rerank_vectors(np.zeros((len(idx), KEY[1]), np.float32)), idx.add(data[:3]))):
        detach()
        with pytest.raises(rq.RabitqError, match=r"exact search needs raw vectors attached \(rbq_bf_set_rerank_vectors\)") as e:
            idx.batch_search_exact_raw(q, rq.BruteForceSearchParams(10), pool=100)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG
    idx.close()
