"""rbq_mstg_range_batch / _device (include/ext/rbq_mstg_range.h) on an MI355X.  Every comparison is exact: lists, ids,
counts and score bits equal the NumPy restatement over the CPU oracle (tests/mstg_range_ref.py, which describes the case).  Seeded."""
import numpy as np
import pytest
import torch

import mstg_range_ref as ref
import rabitq_rs_amd as rq

pytestmark = pytest.mark.gpu
EF, EPS, CAP = 48, 0.6, 1200


def bits_of(got):
    """(ids u64, score bits u32, counts u32[, lists u32, list counts u32]) of a call's arrays or tensors"""
    views = (np.uint64, np.uint32, np.uint32, np.uint32, np.uint32)
    return tuple(np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(v) for a, v in zip(got, views))


@pytest.fixture(scope="module", params=[(m, d) for m in (0, 1) for d in (64, 960)], ids=lambda p: "metric%d_dim%d" % p)
def main(request):
    metric, dim = request.param
    case, q = ref.main_case(metric, dim)
    lists, counts, cands = ref.estimates(case, q, EF, EPS)
    idx = case.device_index()
    yield case, q, idx, lists, counts, cands
    idx.close()


RADII = {"kth20": None, "inf": np.inf, "zero": 0.0, "negative": -1.0, "nan": np.nan}  # kth20: the median 20th-nearest estimate


@pytest.mark.parametrize("distinct", [0, 1])
@pytest.mark.parametrize("radius", list(RADII))
def test_parity_host_and_device_entry(main, radius, distinct):
    case, q, idx, lists, counts, cands = main
    r = ref.kth_estimate_radius(cands) if radius == "kth20" else RADII[radius]
    wi, wb, wc, raw = ref.range_rows(cands, r, distinct, CAP)
    if radius in ("kth20", "inf"):
        assert raw.max() > 256                                  # more matches than one tile of the scan holds
        dup = ref.range_rows(cands, r, 1, CAP)[2].astype(np.int64)
        assert (dup[dup != ref.U32_MAX] < raw[dup != ref.U32_MAX]).any()  # a query's raw matches hold an id twice
    if radius == "inf":  # the last query exceeds the distinct limit and the capacity, its neighbours neither
        assert raw[-1] > ref.DISTINCT_MAX and raw[-1] > CAP and (raw[:-1] <= CAP).all()
        assert wc[-1] == (ref.U32_MAX if distinct else raw[-1]) and (wi[-1] == ref.NONE64).all() == bool(distinct)
    host = bits_of(rq.mstg_range_rows(idx, q, r, CAP, EF, EPS, bool(distinct), return_lists=True))
    dev = bits_of(rq.mstg_range_rows(idx, torch.from_numpy(q).cuda(), r, CAP, EF, EPS, bool(distinct), return_lists=True))
    torch.cuda.synchronize()
    for name, got in (("host", host), ("device", dev)):
        assert np.array_equal(got[4], counts) and np.array_equal(got[3], lists), name
        assert np.array_equal(got[2], wc), (name, got[2], wc)
        assert np.array_equal(got[0], wi), (name, np.nonzero((got[0] != wi).any(axis=1))[0][:10])
        assert np.array_equal(got[1], wb), (name, np.nonzero((got[1] != wb).any(axis=1))[0][:10])


@pytest.mark.parametrize("distinct", [0, 1])
def test_capacity_below_the_total(main, distinct):
    case, q, idx, lists, counts, cands = main
    r = ref.kth_estimate_radius(cands)
    wi, wb, wc, raw = ref.range_rows(cands, r, distinct, 7)
    assert (wc[wc != ref.U32_MAX] > 7).any()
    got = bits_of(rq.mstg_range_rows(idx, q, r, 7, EF, EPS, bool(distinct)))
    assert np.array_equal(got[2], wc) and np.array_equal(got[0], wi) and np.array_equal(got[1], wb)
    zero = rq.mstg_range_rows(idx, q, r, 0, EF, EPS, bool(distinct))      # capacity 0 and ef_search 0: every count 0
    none = rq.mstg_range_rows(idx, q, r, 7, 0, EPS, bool(distinct))
    assert not zero[2].any() and not none[2].any() and (none[0] == ref.NONE64).all() and np.isnan(none[1]).all()


def radius_for_total(est, total):
    """the radius under which exactly `total` of the estimates `est` match (strictly below it)"""
    s = np.sort(est)
    assert total < len(s) and s[total - 1] < s[total]
    return s[total]


@pytest.mark.parametrize("total", [1, 2, 37, ref.DISTINCT_MAX, ref.DISTINCT_MAX + 1])
def test_distinct_at_its_size_edges(main, total):
    """the last query's scan matches exactly `total` entries: one, two (the smallest sort), no power of two, the limit (answered)
    and one more (UINT32_MAX and an empty row); the row without `distinct` is the scan's own, padded from its total"""
    case, q, idx, lists, counts, cands = main
    r = radius_for_total(cands[-1][1], total)
    for distinct in (1, 0):
        wi, wb, wc, raw = ref.range_rows(cands, r, distinct, CAP)
        assert raw[-1] == total
        if distinct:
            assert wc[-1] == (ref.U32_MAX if total > ref.DISTINCT_MAX else len(np.unique(cands[-1][0][cands[-1][1] < r])))
        got = bits_of(rq.mstg_range_rows(idx, q, r, CAP, EF, EPS, bool(distinct)))
        assert np.array_equal(got[2], wc), (got[2], wc)
        assert np.array_equal(got[0], wi) and np.array_equal(got[1], wb)
    if total <= 37:  # a capacity equal to the distinct count: the padding starts at the row's end
        cap = int(ref.range_rows(cands, r, 1, CAP)[2][-1])
        wi, wb, wc, _ = ref.range_rows(cands, r, 1, cap)
        got = bits_of(rq.mstg_range_rows(idx, q[-1:], r, cap, EF, EPS, True))
        assert np.array_equal(got[2], wc[-1:]) and np.array_equal(got[0], wi[-1:]) and np.array_equal(got[1], wb[-1:])


def test_errors_are_the_searchs_in_its_order(main):
    case, q, idx, lists, counts, cands = main
    from rabitq_rs_amd import index as ix
    nq, dim = q.shape
    ids, sc, cnt = np.zeros((nq, 4), np.uint64), np.zeros((nq, 4), np.float32), np.zeros(nq, np.uint32)
    bad = {"dimension": (q.ctypes.data, dim + 16, 4, cnt.ctypes.data), "null buffer after dimension": (None, dim + 16, 4, None),
           "null buffer": (q.ctypes.data, dim, 4, None), "null buffer before capacity": (None, dim, (1 << 20) + 1, cnt.ctypes.data)}
    for why, (qp, qd, k, cp) in bad.items():
        want = ix.lib().rbq_mstg_search_batch(idx._h, qp, nq, qd, k, EF, EPS, ids.ctypes.data, sc.ctypes.data, cp, None, None), ix._detail()
        got = ix.lib_ext().rbq_mstg_range_batch(idx._h, qp, nq, qd, k, EF, EPS, 1.0, 1, ids.ctypes.data, sc.ctypes.data, cp, None, None), ix._detail()
        assert want[0] != 0 and got == want, (why, got, want)
    with pytest.raises(rq.RabitqError, match=r"capacity too large for one call \(capacity <= 2\^20\)"):
        rq.mstg_range_rows(idx, q, 1.0, (1 << 20) + 1, EF, EPS)


def test_chunking_and_repeatability(main):
    case, q, idx, lists, counts, cands = main
    r = ref.kth_estimate_radius(cands)
    for distinct in (False, True):
        want, again = (bits_of(rq.mstg_range_rows(idx, q, r, CAP, EF, EPS, distinct, return_lists=True)) for _ in range(2))
        try:
            idx.set_option("mstg_search_budget", 1)             # one query per chunk: 17 chunks
            cut = bits_of(rq.mstg_range_rows(idx, q, r, CAP, EF, EPS, distinct, return_lists=True))
        finally:
            idx.set_option("mstg_search_budget", 0)
        for a, b, c in zip(want, again, cut):
            assert np.array_equal(a, b) and np.array_equal(a, c)


def test_f16_queries_equal_the_widened_rows(main):
    case, q, idx, lists, counts, cands = main
    q16, r = q.astype(np.float16), ref.kth_estimate_radius(cands)
    want = bits_of(rq.mstg_range_rows(idx, q16.astype(np.float32), r, CAP, EF, EPS, True, return_lists=True))
    got = bits_of(rq.mstg_range_rows(idx, q16, r, CAP, EF, EPS, True, return_lists=True))
    assert want[2].any()
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


def test_binding(main):
    case, q, idx, lists, counts, cands = main
    r = ref.kth_estimate_radius(cands)
    wi, wb, wc, _ = ref.range_rows(cands, r, 1, CAP)
    lims, ids, dist = rq.mstg_range_search(idx, q, r, EF, EPS)  # (rows of 1024 first; a total beyond that repeats the call)
    assert np.array_equal(np.diff(lims), wc)
    for i in range(len(q)):
        assert np.array_equal(ids[lims[i]:lims[i + 1]], wi[i, :wc[i]])
        assert np.array_equal(dist[lims[i]:lims[i + 1]].view(np.uint32), wb[i, :wc[i]])
    with pytest.raises(rq.RabitqError, match="RBQ_MSTG_RANGE_DISTINCT_MAX"):
        rq.mstg_range_search(idx, q, np.inf, EF, EPS)
    m = rq.MstgIndex(case.x.shape[1], "euclidean" if case.metric == 0 else "angular", default_ef_search=EF, pruning_epsilon=EPS)
    m.handle = idx
    assert [len(x) for x in m.range_query(q, r)] == wc.tolist()
