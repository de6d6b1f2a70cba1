"""tests/range_ref.py (the range search restated over the oracle) against the oracle's own top-k search.  No GPU."""
import numpy as np
import pytest

import oracle
import range_ref
from conftest import build_index, make_dataset

F32 = np.float32


def _case(bits, metric, n=3000, dim=96, nlist=12, nq=8):
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, normalize=(metric == 1), seed=2900 + bits + metric)
    q = np.ascontiguousarray(make_dataset(nq, dim, max(nlist // 4, 1), 2950 + bits, normalize=(metric == 1)), dtype=F32)
    return data, built, q


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_unbounded_radius_is_the_full_search(bits, metric):
    """R = +inf and every list probed: the matches are what the top-k search returns at top_k = n, as a set with its scores"""
    data, built, q = _case(bits, metric, n=1200, nq=4)
    n, nlist = len(data), built.n_lists
    try:
        rc, oids, osc, ocnt, _ = oracle.search_batch(built, q, n, nlist)
        assert rc == 0
        ref = range_ref.range_batch(built, q, F32(np.inf) if metric == 0 else F32(-np.inf), nlist)
        for i, (ids, sc, (est, skipped, ext)) in enumerate(ref):
            c = int(ocnt[i])
            assert len(ids) == c == est and skipped == 0 and ext == (n if bits > 1 else 0)
            a = np.lexsort((sc.view(np.uint32), ids))
            b = np.lexsort((osc[i, :c].view(np.uint32), oids[i, :c]))
            assert np.array_equal(ids[a], oids[i, :c][b])
            assert np.array_equal(sc[a].view(np.uint32), osc[i, :c][b].view(np.uint32))
    finally:
        built.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_radius_at_the_kth_distance_gives_the_first_k(bits, metric):
    """R = the bits of the (k+1)-th distance: the matches, sorted, are the first k results (distinct distances) — but for a result
    whose own lower bound is >= R: the top-k search met it while its running threshold was still above R and evaluated it, the
    range search skips it (step 3 of the loop; the bound is an estimate's, and a refined distance may lie below it).  Such
    results are identified through their bounds and are few.  The data set exercises every branch: vectors skipped by the
    bound, refined and rejected, matched."""
    data, built, q = _case(bits, metric)
    nprobe = 6
    try:
        for k in (5, 20, 49):
            rc, oids, osc, ocnt, _ = oracle.search_batch(built, q[:1], k + 1, nprobe)
            assert rc == 0 and ocnt[0] == k + 1
            d = osc[0] if metric == 0 else -osc[0]
            assert len(np.unique(d)) == k + 1, "the test needs distinct distances"
            ref = range_ref.range_batch(built, q, range_ref.kth_distance_radius(built, q[0], k + 1, nprobe), nprobe)
            ids, sc, _ = ref[0]
            R = range_ref.internal_radius(metric, range_ref.kth_distance_radius(built, q[0], k + 1, nprobe))
            lb_of = {int(i): b for pi, pb, _ in range_ref.probed_vectors(built, q[0], nprobe) for i, b in zip(pi, pb)}
            below = np.array([not (lb_of[int(i)] >= R) for i in oids[0, :k]])
            assert below.sum() >= k - 2, "more than two of the first k results have a lower bound at or above R"
            o = np.argsort(sc if metric == 0 else -sc, kind="stable")
            assert np.array_equal(ids[o], oids[0, :k][below])
            assert np.array_equal(sc[o].view(np.uint32), osc[0, :k][below].view(np.uint32))
            dg = range_ref.diag_of(ref).astype(np.int64)
            tot = np.array([len(r[0]) for r in ref])
            assert dg[:, 1].sum() > 0, "vectors skipped by the bound"
            assert (dg[:, 0] - tot).sum() > 0, "vectors that were refined and rejected"
    finally:
        built.close()


def test_nan_radius_and_filter():
    data, built, q = _case(7, 0, n=1200, nq=3)
    try:
        ref = range_ref.range_batch(built, q, F32(np.nan), 6)
        for ids, sc, (est, skipped, ext) in ref:
            assert len(ids) == 0 and skipped == 0 and ext >= est > 0
        allowed = set(range(0, len(data), 3))
        r = range_ref.kth_distance_radius(built, q[0], 40, 6)
        full = range_ref.range_batch(built, q, r, 6)
        filt = range_ref.range_batch(built, q, r, 6, allowed)
        for (fi, fs, _), (gi, gs, gd) in zip(full, filt):
            m = np.isin(fi, np.fromiter(allowed, np.uint64))
            assert np.array_equal(fi[m], gi) and np.array_equal(fs[m].view(np.uint32), gs.view(np.uint32))
    finally:
        built.close()
