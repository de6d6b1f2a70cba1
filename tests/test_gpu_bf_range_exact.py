"""The exact brute-force range search (rbq_bf_range_exact_batch: k_bf_dist -> k_bf_range_exact -> k_bf_range_place; DESIGN.md
section 41) against its restatement (tests/bf_range_exact_ref.py), every comparison exact: ids, score bits, totals and the unused
slots of every row.  x is an element of the reference's own exact distances, so the strict < is covered.  Seeded."""
import functools

import numpy as np
import pytest
import torch

import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, bruteforce as bfm
import bf_range_exact_ref as xref
import bf_ref
import rerank_pool_ref

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
DIMS = (7, 20, 33, 64, 136)  # scalar tail only; main part + tail; odd (16-bit rows by element); one 16-bit span; past one f32 step
RAWS = ("f32", "f16", "bf16")
BIG = 2 * 2048 + 37          # three spans of kBfRangeSpan, the last partial
KEY = (1100, 20, 7, 0, "f16")


@functools.lru_cache(maxsize=None)
def case(n, dim, bits, metric, nq=33):
    """(index, prep, queries, estimates [nq][n], data); the queries are spread along the data's mean so that the totals differ"""
    rng = np.random.default_rng(1000 * bits + 10 * metric + dim)
    data = (rng.standard_normal((n, dim)) + 1.0).astype(np.float32)
    q = (rng.standard_normal((nq, dim)) + np.roll(np.linspace(-1, 1, nq), -(nq // 2))[:, None]).astype(np.float32)
    built = rq.builder.train_bruteforce(data, bits, metric, 1, 7, True)
    prep = bf_ref.Prepared(built.hdr_ptr, built.arrays())
    est = np.stack([bf_ref.distances(prep, x).astype(np.float32) for x in q])
    return rq.BruteForceRabitqIndex.from_built(built), prep, q, est, data


@functools.lru_cache(maxsize=None)
def rows_of(n, dim, bits, metric, raw, nq=33):
    """(rows as attached, attach dtype, rows widened, exact scores [nq][n], exact distances [nq][n]) of a case"""
    q, data = case(n, dim, bits, metric, nq)[2::2]
    stored, dtype, wide = xref.stored_rows(data, raw)
    full = np.stack([rerank_pool_ref.exact_scores(x, wide, range(n), metric) for x in q])
    return stored, dtype, wide, full, (full if metric == 0 else -full)


def attached(*key):  # (the case's index with its rows of key's element type attached, the queries)
    idx, _, q = case(*key[:4], *key[5:])[:3]
    idx.set_rerank_vectors(*rows_of(*key)[:2])
    assert idx.rerank_dtype() == key[4]
    return idx, q


def rows(idx, q, r, x, cap, chunk=0, words=None, nbits=0):
    """range_rows' exact mode with at most `chunk` vectors per chunk (0: no limit); the scores as bit patterns"""
    assert bfm.lib().rbq_bf_debug_set_chunk_vectors(chunk) == 0
    try:
        ids, sc, tot = idx.range_rows(q, r, cap, words, nbits, exact_x=x)
    finally:
        bfm.lib().rbq_bf_debug_set_chunk_vectors(0)
    return ids, sc.view(np.uint32), tot


def expect(key, r, x, cap, allowed=None):  # the restatement's (ids, score bits, totals), and the candidates per query
    _, prep, q, est, _ = case(*key[:4], *key[5:])
    wide, full = rows_of(*key)[2:4]
    per = [xref.row(prep, q[i], wide, r, x, cap, allowed, est[i], full[i]) for i in range(len(q))]
    return tuple(np.array([p[k] for p in per], t) for k, t in enumerate((np.uint64, np.uint32, np.uint32))), np.array([p[3] for p in per])


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


def radii(key):
    """x: query 0's 100th smallest exact distance; the candidate radii (r, x, vector chunk): r = x, up to about 1.2 x, +inf in the
    case's chunks and in one chunk, and last one so small that query 0 has a single candidate, with an x of that candidate set's own"""
    est, dist = case(*key[:4], *key[5:])[3], rows_of(*key)[4]
    x, small, chunk = np.sort(dist[0])[99], np.sort(est[0])[1], 700 if key[0] == 1100 else 0
    xs = np.sort(dist[np.isfinite(est) & (est < small)])
    return [(x, x, chunk), (np.float32(x + 0.2 * abs(x)), x, chunk), (INF, x, chunk), (INF, x, 0), (small, xs[len(xs) // 2], chunk)]


def visible(want, ncand):  # the exact score accepts a candidate and rejects one: without both the exact stage would not show
    return want[2].sum() > 0 and (ncand - want[2].astype(np.int64)).sum() > 0


# every dimension x element type x metric at 1100 vectors in chunks of 700 and 400, the ex bits alternating; three spans in one
# chunk for every element type; 1025 queries (two sub-batches) at the smallest dimension
KEYS = [(1100, d, (7, 1)[(i + m) % 2], m, raw) for i, d in enumerate(DIMS) for m in (0, 1) for raw in RAWS] + \
       [(BIG, 20, (7, 1)[i % 2], i % 2, raw) for i, raw in enumerate(RAWS)] + [(300, 7, 7, 0, "bf16", 1025)]


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_parity(key):
    idx, q = attached(*key)
    for k, (r, x, chunk) in enumerate(radii(key)):
        want, ncand = expect(key, r, x, 64)
        assert visible(want, ncand), (r, x)
        if r == INF:
            assert (ncand == key[0]).all()                # 1100 in one span: 35 scoring passes, the last with 12 groups
        elif k == 4:
            assert ncand[0] == 1                          # a span of query 0 without a candidate: no pass
        assert same(rows(idx, q, r, x, 64, chunk), want), (r, x, chunk)
    if key[4] != "f32":                                   # 16-bit rows answer as the widened rows attached as f32
        r, x, chunk = radii(key)[1]
        got = rows(idx, q, r, x, 64, chunk)
        idx.set_rerank_vectors(rows_of(*key)[2])
        assert idx.rerank_dtype() == "f32" and same(rows(idx, q, r, x, 64, chunk), got)


def test_filter_shorter_than_the_index():
    (idx, q), x = attached(*KEY), radii(KEY)[0][1]
    allowed = np.zeros(1100, bool)
    allowed[:900] = np.random.default_rng(5).random(900) < 0.5
    words, nbits = bfm._filter_words(np.nonzero(allowed)[0])
    want, ncand = expect(KEY, INF, x, 64, allowed)
    assert nbits < 1100 and (ncand == allowed.sum()).all() and visible(want, ncand)  # only what the filter lets through is scored
    assert same(rows(idx, q, INF, x, 64, 700, words, nbits), want)


@pytest.mark.parametrize("cap", [64, 0, 1500], ids=["cut", "count_only", "above_n"])
def test_capacities_the_same_bytes_twice_and_the_other_calls_untouched(cap):
    (idx, q), (r, x, chunk) = attached(*KEY), radii(KEY)[2]
    want, est_r = expect(KEY, r, x, cap)[0], case(*KEY[:4])[3][0, 500]
    assert (want[2] > 64).any() and (want[2] <= 64).any()
    before = idx.batch_search_raw(q, rq.BruteForceSearchParams(10)), idx.range_rows(q, est_r, 64)
    got = rows(idx, q, r, x, cap, chunk)  # (range_rows passes NULL rows at capacity 0)
    assert same(got, want) and same(rows(idx, q, r, x, cap, chunk), got)
    assert np.array_equal(idx.count_in_range(q, x, exact=True), want[2])
    assert same(idx.batch_search_raw(q, rq.BruteForceSearchParams(10)), before[0]) and same(idx.range_rows(q, est_r, 64), before[1])


def test_state_of_the_handle():
    (q, data), (r, x, _), (stored, dtype) = case(*KEY[:4])[2::2], radii(KEY)[1], rows_of(*KEY)[:2]
    idx = rq.BruteForceRabitqIndex.train(data, KEY[2], KEY[3], 1, 7, True)
    with pytest.raises(rq.RabitqError, match="raw vectors attached") as e:
        idx.range_rows(q, r, 64, exact_x=x)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and idx.rerank_dtype() is None
    idx.set_rerank_vectors(stored, dtype=dtype)
    want = expect(KEY, r, x, 64)[0]
    with pytest.raises(rq.RabitqError, match="1099 rows for an index of 1100"):
        idx.set_rerank_vectors(stored[:-1], dtype=dtype)
    assert idx.rerank_dtype() == "f16" and same(rows(idx, q, r, x, 64), want)  # the handle keeps its rows
    t = torch.from_numpy(stored.view(np.float16)).cuda()                       # borrowed: the host copy's bytes
    idx.set_rerank_vectors(t)
    assert idx._raw_keep is t and idx.rerank_dtype() == "f16" and same(rows(idx, q, r, x, 64), want)
    idx.set_rerank_vectors(None)
    assert idx.rerank_dtype() is None and idx._raw_keep is None
    for mutate in (lambda: idx.add(data[:3]), lambda: idx.remove_ids([0, 1, 2])):
        idx.set_rerank_vectors(np.zeros((len(idx), KEY[1]), np.float32))
        mutate()
        with pytest.raises(rq.RabitqError, match="raw vectors attached"):
            idx.count_in_range(q, x, exact=True)
        assert idx.rerank_dtype() is None
    idx.close()


def test_reattach_and_detach():
    """f32 host rows, f16 host rows over them, a borrowed bf16 tensor over those, then none: after every step the element type, and
    every vector scored against the rows as they are then (the rows replaced are gone, borrowed ones are not freed)"""
    n, dim = 100, 24
    q, data = case(n, dim, 7, 0)[2::2]
    idx = rq.BruteForceRabitqIndex.train(data, 7, 0, 1, 7, True)
    x = np.sort(rows_of(n, dim, 7, 0, "f32")[4][0])[n // 2]
    for raw in RAWS:
        stored, dtype = rows_of(n, dim, 7, 0, raw)[:2]
        if raw == "bf16":
            stored = torch.from_numpy(stored.view(np.int16)).view(torch.bfloat16).cuda()
        idx.set_rerank_vectors(stored, dtype=None if raw == "bf16" else dtype)
        want, ncand = expect((n, dim, 7, 0, raw), INF, x, 64)
        assert (idx._raw_keep is stored) == (raw == "bf16") and idx.rerank_dtype() == raw
        assert (ncand == n).all() and visible(want, ncand) and same(rows(idx, q, INF, x, 64), want), raw
    idx.set_rerank_vectors(None)
    assert idx.rerank_dtype() is None and idx._raw_keep is None
    with pytest.raises(rq.RabitqError, match=r"exact range search needs raw vectors attached \(rbq_bf_set_rerank_vectors\)") as e:
        idx.range_rows(q, INF, 64, exact_x=x)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    idx.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_python_layer(metric):
    key = (1100, 20, 7, metric, "f32")
    (idx, q), (r, x, _) = attached(*key), radii(key)[1]
    per = expect(key, r, x, 1100)[0]
    ux, ur = (x, r) if metric == 0 else (-x, -r)  # inner product: score > radius is distance < -radius
    lims, ids, sc = idx.range_search(q, ux, exact=True, candidate_radius=ur)
    assert np.array_equal(lims, np.cumsum(np.r_[0, per[2]])) and (per[2] > 0).any()
    assert np.array_equal(ids, per[0][per[0] != xref.U64MAX]) and np.array_equal(sc.view(np.uint32), per[1][per[0] != xref.U64MAX])
    assert np.array_equal(idx.count_in_range(q, ux, exact=True, candidate_radius=ur), per[2])
    assert np.array_equal(idx.count_in_range(q, ux, exact=True), expect(key, INF, x, 0)[0][2])  # None: every vector is scored
