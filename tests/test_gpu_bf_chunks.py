"""The brute-force search's several-chunk path and its full global-memory heap (api_bf.hip, bf.hpp), which no index of a
testable size reaches by itself: rbq_bf_debug_set_chunk_vectors caps the vectors per chunk, so that k_bf_select carries its heap
from chunk to chunk (written at a chunk's end, reloaded and `ptie` recomputed at the next one's start, ids formed from v0) and
k_bf_dist addresses codes, factors and filter bits by v0 + vl.  Every capped call is compared with the numpy restatement
(tests/bf_ref.py) and, byte for byte and push for push, with the same call without a cap; rbq_bf_debug_select_launches shows
that the chunks ran."""
import threading

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import bruteforce as bfm
from test_gpu_bruteforce import U64MAX, check, make

pytestmark = pytest.mark.gpu

DIST_BUDGET, HEAP_BUDGET, OUT_BUDGET, MAX_SUB, LDS_HEAP_MAX_TOP_K = 128 << 20, 48 << 20, 48 << 20, 1024, 8191


def _ceil(a, b):
    return -(-a // b)


def _launches(n, nq, k, cap):
    """k_bf_select launches of one call: (query sub-batches) x (vector chunks), from the plan of bf_search_impl.  The cap
    shortens the chunks only; the sub-batch still comes from the workspace budgets."""
    nv_chunk = min(n, DIST_BUDGET // 4, cap or n)
    n_chunks = _ceil(n, nv_chunk)
    sub = min(nq, MAX_SUB, max(1, DIST_BUDGET // (nv_chunk * 4)), max(1, OUT_BUDGET // (k * 12)))
    if n_chunks > 1 or k > LDS_HEAP_MAX_TOP_K:
        sub = min(sub, max(1, HEAP_BUDGET // ((k + 1) * 8)))
    return _ceil(nq, sub) * n_chunks


def _call(idx, prep, q, k, cap, *args, **kw):
    """`check` under a cap of `cap` vectors per chunk (0: none): (ids, scores, counts), (pushes, tie pushes), launches"""
    L = bfm.lib()
    prev = L.rbq_bf_debug_set_chunk_vectors(cap)
    try:
        s0, l0 = idx.heap_stats(), L.rbq_bf_debug_select_launches()
        out = check(idx, prep, q, k, *args, **kw)
        s1, l1 = idx.heap_stats(), L.rbq_bf_debug_select_launches()
    finally:
        L.rbq_bf_debug_set_chunk_vectors(0)
    assert prev == 0  # (no earlier test left a cap behind)
    return out, (s1["pushes"] - s0["pushes"], s1["tie_pushes"] - s0["tie_pushes"]), l1 - l0


def _same_bytes(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def _chunked_equals_unchunked(idx, prep, q, k, caps, *args, **kw):
    """the reference, the bytes of the call without a cap, its pushes and tie pushes, and the launch count, for every cap"""
    n, nq = len(idx), len(q)
    base, base_stats, launches = _call(idx, prep, q, k, 0, *args, **kw)
    assert launches == _launches(n, nq, k, 0), (launches, n, nq, k)
    for cap in caps:
        got, stats, launches = _call(idx, prep, q, k, cap, *args, **kw)
        assert launches == _launches(n, nq, k, cap), (launches, n, nq, k, cap)
        assert _same_bytes(got, base), (k, cap)
        assert stats == base_stats, (k, cap, stats, base_stats)  # (the skip rule does not depend on where the chunks fall)
    return base, base_stats


def test_launch_plan_of_the_cases_below():
    """the counts the tests expect, spelled out: the cap multiplies the chunks and leaves the sub-batch alone"""
    assert [_launches(700, 9, 10, c) for c in (0, 64, 65, 511, 512, 513, 699, 700, 701)] == [1, 11, 11, 2, 2, 2, 2, 1, 1]
    assert _launches(500, 7, 10, 96) == 6 and _launches(1200, 4, 20, 100) == 12 and _launches(2000, 20, 100, 333) == 7
    assert _launches(20000, 3, 16384, 0) == 1 and _launches(20000, 3, 8191, 4096) == 5 and _launches(10000, 3, 9000, 4096) == 3
    assert _launches(40, 257, 16384, 0) == 2 and _launches(40, 257, 16384, 16) == 6 and _launches(5000, 200, 10, 1024) == 5


@pytest.fixture(scope="module")
def idx700():
    return make(700, 64, 7, 0, 1, 700)


@pytest.mark.parametrize("k", [1, 10, 100, 300, 1000])
def test_chunk_boundaries(idx700, k):
    """512 is one read group of k_bf_select; 700 and 701 give a single chunk; at top_k 300 the heap is still filling when a
    chunk ends, at 1000 it never fills; nine queries leave the kBfQ query tile ragged"""
    data, built, idx, prep = idx700
    q = np.random.default_rng(k).standard_normal((9, 64)).astype(np.float32)
    _chunked_equals_unchunked(idx, prep, q, k, (64, 65, 511, 512, 513, 699, 700, 701))


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("rotator,dim", [(1, 128), (0, 32)])
def test_matrix_under_a_cap_of_96(bits, metric, rotator, dim):
    data, built, idx, prep = make(500, dim, bits, metric, rotator, 20 * bits + metric + dim)
    q = np.random.default_rng(dim + bits).standard_normal((7, dim)).astype(np.float32)
    _chunked_equals_unchunked(idx, prep, q, 10, (96,))
    _chunked_equals_unchunked(idx, prep, q[:1], 100, (96,))


@pytest.mark.parametrize("metric", [0, 1])
def test_duplicates_across_chunk_boundaries(metric):
    """copies of a vector in different chunks: the heap's tie path with `ptie` recomputed from a reloaded heap"""
    data, built, idx, prep = make(2000, 64, 3, metric, 1, 191 + metric, dup=1500)
    q = np.concatenate([data[:10], np.random.default_rng(2).standard_normal((10, 64)).astype(np.float32)])
    for k in (1, 10, 100):
        _, (pushes, ties) = _chunked_equals_unchunked(idx, prep, q, k, (64, 333))
        assert pushes > 0 and ties > 0, (k, pushes, ties)


@pytest.mark.parametrize("metric", [0, 1])
def test_filters_under_a_cap_of_100(metric):
    data, built, idx, prep = make(1200, 64, 7, metric, 1, 15 + metric)
    n = 1200
    q = np.random.default_rng(9).standard_normal((4, 64)).astype(np.float32)
    rng = np.random.default_rng(3)
    # (the last set: filter_nbits < n, and every chunk from vector 700 on is filtered out as a whole)
    for allowed_ids in ([], list(range(n)), sorted(set(rng.integers(0, n, 300).tolist())), list(range(0, 700, 3))):
        mask = np.zeros(n, bool)
        mask[allowed_ids] = True
        words, nbits = bfm._filter_words(allowed_ids)
        (ids, scores, counts), _ = _chunked_equals_unchunked(idx, prep, q, 20, (100,), mask, words, nbits)
        assert np.all(counts == min(20, len(allowed_ids)))


def test_non_finite_query_under_a_cap():
    data, built, idx, prep = make(300, 64, 7, 0, 1, 18)
    for bad in (np.inf, np.nan, -np.inf):
        q = np.random.default_rng(1).standard_normal((3, 64)).astype(np.float32)
        q[1, 5] = bad
        (ids, scores, counts), _ = _chunked_equals_unchunked(idx, prep, q, 10, (64,))
        assert list(counts) == [10, 0, 10]


@pytest.mark.parametrize("n,dup", [(10000, 0), (20000, 0), (10000, 4000)])
def test_global_heap_with_evictions(n, dup):
    """top_k 8191 is the largest LDS heap (64 KiB of dynamic LDS), 8192 the first heap in global memory; with n above top_k the
    heap fills, so candidates are popped and skipped and path_tie reads what lane 0 has just written; under the cap of 4096 the
    global heap fills across chunks"""
    data, built, idx, prep = make(n, 64, 7, 0, 1, n + dup, dup=dup)
    q = np.random.default_rng(n).standard_normal((3, 64)).astype(np.float32)
    if dup:
        q[0] = data[1]
    for k in (8191, 8192, 9000, 16384):
        (ids, scores, counts), (pushes, ties) = _chunked_equals_unchunked(idx, prep, q, k, (4096,))
        assert np.all(counts == min(n, k))
        assert pushes >= 3 * min(n, k) and (pushes > 3 * k) == (n > k), (n, k, pushes)  # (evictions wherever n > top_k)
        print(f"n={n} dup={dup} top_k={k}: pushes={pushes} tie_pushes={ties}")


def test_sub_batches_from_the_output_budget():
    """top_k 16384 allows 256 queries per sub-batch: query 256 is alone in the second one"""
    data, built, idx, prep = make(40, 64, 7, 0, 1, 40)
    q = np.random.default_rng(5).standard_normal((257, 64)).astype(np.float32)
    (ids, scores, counts), _ = _chunked_equals_unchunked(idx, prep, q, 16384, (0, 16), sample=[0, 255, 256])
    assert np.all(counts == 40)
    assert np.all(np.sort(ids[:, :40], axis=1) == np.arange(40, dtype=np.uint64))
    assert not np.isnan(scores[:, :40]).any()
    assert np.all(ids[:, 40:] == U64MAX) and np.all(np.isnan(scores[:, 40:]))


def test_two_threads_on_one_handle_under_a_cap():
    data, built, idx, prep = make(5000, 128, 7, 1, 1, 112)
    rng = np.random.default_rng(4)
    qs = [rng.standard_normal((200, 128)).astype(np.float32) for _ in range(4)]
    params = rq.BruteForceSearchParams(10)
    plain = [idx.batch_search_raw(q, params) for q in qs]
    out = [None] * 4

    def run(i):
        out[i] = idx.batch_search_raw(qs[i], params)
    L = bfm.lib()
    assert L.rbq_bf_debug_set_chunk_vectors(1024) == 0  # (process-wide: set before the threads start)
    try:
        l0 = L.rbq_bf_debug_select_launches()
        serial = [idx.batch_search_raw(q, params) for q in qs]
        th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        launches = L.rbq_bf_debug_select_launches() - l0
    finally:
        L.rbq_bf_debug_set_chunk_vectors(0)
    assert launches == 8 * _launches(5000, 200, 10, 1024) == 40
    for a, b, c in zip(plain, serial, out):
        assert _same_bytes(a, b) and _same_bytes(a, c)
    check(idx, prep, qs[0][:3], 10)
