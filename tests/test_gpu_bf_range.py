"""The brute-force range search (rbq_bf_range_batch: k_bf_dist -> k_bf_range_count -> k_bf_range_place) against its restatement
(tests/bf_range_ref.py over tests/bf_ref.py), every comparison exact: ids, score bits, totals and the unused slots of every row.
The data has a mean and the queries a varying component along it, so that one radius leaves some rows short and cuts others."""
import functools

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import bruteforce as bfm
import bf_range_ref
import bf_ref

pytestmark = pytest.mark.gpu

SPAN = 2048  # kBfRangeSpan
INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def case(n, dim, bits, metric, nq=33):
    """(index, prep, queries, reference distances [nq][n]); query 0 sits in the middle of the queries' spread"""
    rng = np.random.default_rng(1000 * bits + 10 * metric + dim)
    data = (rng.standard_normal((n, dim)) + 1.0).astype(np.float32)
    q = (rng.standard_normal((nq, dim)) + np.roll(np.linspace(-1, 1, nq), -(nq // 2))[:, None]).astype(np.float32)
    built = rq.builder.train_bruteforce(data, bits, metric, 1, 7, True)  # (FHT-Kac rotator: dim 40 is padded to 64)
    prep = bf_ref.Prepared(built.hdr_ptr, built.arrays())
    dist = np.stack([bf_ref.distances(prep, x).astype(np.float32) for x in q])
    return rq.BruteForceRabitqIndex.from_built(built), prep, q, dist


def rows(idx, q, r, cap, chunk=0, words=None, nbits=0):
    """range_rows with at most `chunk` vectors per chunk (0: no limit)"""
    L = bfm.lib()
    assert L.rbq_bf_debug_set_chunk_vectors(chunk) == 0
    try:
        return idx.range_rows(q, r, cap, words, nbits)
    finally:
        L.rbq_bf_debug_set_chunk_vectors(0)


def expect(prep, q, dist, r, cap, allowed=None):
    per = [bf_range_ref.row(prep, q[i], r, cap, allowed, dist[i]) for i in range(len(q))]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.array([p[2] for p in per], np.uint32)


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


def median_of(dist):
    return np.sort(dist[0])[dist.shape[1] // 2]  # an element of query 0's distances: that vector sits exactly at r


# chunks of 700 and 400 vectors (a span is wider than the index), and once three spans in one chunk, the last one partial
@pytest.mark.parametrize("n,chunk,bits,metric", [(1100, 700, b, m) for b in (1, 3, 7) for m in (0, 1)] + [(2 * SPAN + 37, 0, 3, 0)])
def test_parity(n, chunk, bits, metric):
    idx, prep, q, dist = case(n, 40 if metric == 0 else 128, bits, metric)
    r = median_of(dist)
    ids, sc, tot = want = expect(prep, q, dist, r, 64)
    assert (tot > 64).any() and (tot <= 64).any()  # rows of both kinds at this radius
    assert tot[0] == n // 2 and np.isfinite(dist[0]).all()             # the vector at r itself is out: strict <
    assert same(rows(idx, q, r, 64, chunk), want)
    got = rows(idx, q, -INF, 64, chunk)
    assert not got[2].any() and (got[0] == bf_range_ref.U64MAX).all() and np.isnan(got[1]).all()
    got = rows(idx, q, INF, 64, chunk)
    assert same(got, expect(prep, q, dist, INF, 64)) and np.array_equal(got[2], np.isfinite(dist).sum(1))


def test_chunks_of_300_carry_the_totals():
    idx, prep, q, dist = case(1100, 40, 3, 0)
    r = median_of(dist)
    one = rows(idx, q, r, 64)
    assert same(rows(idx, q, r, 64, 300), one) and same(one, expect(prep, q, dist, r, 64))


def test_filter_shorter_than_the_index():
    idx, prep, q, dist = case(1100, 40, 3, 0)
    allowed = np.zeros(1100, bool)
    allowed[:900] = np.random.default_rng(5).random(900) < 0.5
    words, nbits = bfm._filter_words(np.nonzero(allowed)[0])
    assert nbits < 1100
    for r in (median_of(dist), INF):
        assert same(rows(idx, q, r, 64, 0, words, nbits), expect(prep, q, dist, r, 64, allowed))


def test_more_queries_than_one_sub_batch():
    idx, prep, q, dist = case(600, 40, 3, 0, nq=1025)
    r = median_of(dist)
    got, want = rows(idx, q, r, 64), expect(prep, q, dist, r, 64)
    assert same(got, want)
    assert same(rows(idx, q[-1:], r, 64), [x[-1:] for x in want])


def test_count_only_with_null_rows():
    idx, prep, q, dist = case(1100, 40, 3, 0)
    r = median_of(dist)
    tot = rows(idx, q, r, 64)[2]
    for chunk in (0, 300):
        ids, sc, cnt = rows(idx, q, r, 0, chunk)  # (range_rows passes NULL rows at capacity 0)
        assert ids.shape == sc.shape == (33, 0) and np.array_equal(cnt, tot)
    assert np.array_equal(idx.count_in_range(q, r), tot)


@pytest.mark.parametrize("metric", [0, 1])
def test_python_layer(metric):
    idx, prep, q, dist = case(1100, 40 if metric == 0 else 128, 3, metric)
    r = np.sort(dist[0])[-1]  # all of query 0 but its farthest vector
    per = [bf_range_ref.row(prep, q[i], r, None, None, dist[i]) for i in range(len(q))]
    assert max(p[2] for p in per) > 1024  # the first call's rows of 1024 are too short
    radius = r if metric == 0 else -r    # inner product: score > radius is distance < -radius
    lims, ids, sc = idx.range_search(q, radius)
    assert np.array_equal(lims, np.cumsum([0] + [p[2] for p in per]))
    assert np.array_equal(ids, np.concatenate([p[0] for p in per]))
    assert np.array_equal(sc.view(np.uint32), np.concatenate([p[1] for p in per]).view(np.uint32))
    lims_s, ids_s, sc_s, tot = idx.range_search(q, radius, max_results=2000, sort=True)
    assert np.array_equal(lims_s, lims) and np.array_equal(tot, np.diff(lims))
    for i, (pid, psc, _) in enumerate(per):
        o = np.lexsort((pid, psc))  # by (score, id)
        assert np.array_equal(ids_s[lims[i]:lims[i + 1]], pid[o]) and np.array_equal(sc_s[lims[i]:lims[i + 1]], psc[o])
    assert np.array_equal(idx.count_in_range(q, radius), tot)


def test_same_bytes_twice_and_the_search_untouched():
    idx, prep, q, dist = case(1100, 40, 3, 0)
    r = median_of(dist)
    before = idx.batch_search_raw(q, rq.BruteForceSearchParams(10))
    assert same(rows(idx, q, r, 64, 300), rows(idx, q, r, 64, 300))
    assert same(idx.batch_search_raw(q, rq.BruteForceSearchParams(10)), before)
