"""The exact MSTG range search (options "mstg_range_exact" / "mstg_range_exact_bits" on rbq_mstg_range_batch / _device;
k_mstg_range_exact.hip) on an MI355X.  Every comparison is exact: lists, ids, counts and the bits of the exact
distances equal the restatement tests/mstg_range_exact_ref.py over the case of tests/mstg_range_ref.py.  MSTG handles take only
dimensions that are multiples of 16, so the scorer's element path is reached by f16 rows borrowed at an address 2 mod 4.  Seeded."""
import functools

import numpy as np
import pytest
import torch

import mstg_range_exact_ref as xref
import mstg_range_ref as ref
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi

pytestmark = pytest.mark.gpu
EF, EPS, CAP, OFF = 48, 0.6, 1200, (0, 0x7F800000)


@functools.lru_cache(maxsize=None)
def base(metric):
    case, q = ref.main_case(metric, 64)
    return (case, q) + ref.estimates(case, q, EF, EPS)


def attach(idx, x, raw):
    """attach rows of type `raw` ("f16@2": f16 rows borrowed at 2 mod 4, kept alive on the handle); returns the rows widened to f32"""
    stored, wide = xref.stored_rows(x, "f16" if raw == "f16@2" else raw)
    if raw != "f16@2":
        idx.set_rerank_vectors(stored, dtype=raw)
        return wide
    buf = torch.full((stored.size + 3,), 0x7e00, dtype=torch.int16, device="cuda")  # (NaN guards around the rows)
    buf[1:1 + stored.size] = torch.from_numpy(stored.view(np.int16).reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert (buf.data_ptr() + 2) % 4 == 2
    idx.set_rerank_vectors(device_ptr=buf.data_ptr() + 2, n=len(x), dtype="f16")
    idx._borrowed = buf
    return wide


@pytest.fixture(scope="module", params=[(m, raw) for m in (0, 1) for raw in ("f32", "f16", "bf16", "f16@2")], ids=lambda p: "metric%d_%s" % p)
def main(request):
    metric, raw = request.param
    case, q, lists, counts, cands = base(metric)
    idx = case.device_index()
    wide = attach(idx, case.x, raw)
    r = ref.kth_estimate_radius(cands, 50)
    x = xref.kth_exact_radius(cands, q, wide, metric, r, 20)
    yield case, q, idx, raw, r, x, lambda r=r, x=x, cap=CAP, rows=wide: xref.exact_rows(cands, q, rows, metric, r, x, cap) + (lists, counts)
    idx.close()


def options(idx):
    return tuple(int(idx.debug_copy_index(n, np.empty(1, np.int32))[0]) for n in ("mstg_range_exact", "mstg_range_exact_bits"))


def call(idx, q, r, x, cap=CAP, want=None):
    """the exact call's arrays as bit patterns; compared with the restatement's rows `want` where given"""
    got = rq.mstg_range_rows(idx, q, x, cap, EF, EPS, True, return_lists=True, exact=True, candidate_radius=r)
    torch.cuda.synchronize()
    got = tuple(np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(v) for a, v in zip(got, (np.uint64,) + (np.uint32,) * 4))
    assert options(idx) == OFF                                   # put back after the call
    for k in (2, 0, 1, 3, 4) if want is not None else ():
        assert np.array_equal(got[k], want[k + (k > 2)]), (k, got[k], want[k + (k > 2)])
    return got


@pytest.mark.parametrize("entry", ["host", "device"])
def test_parity_capacity_overflow_and_nan_radius(main, entry):
    case, q, idx, raw, r, x, want_of = main
    want, want7, over = want_of(), want_of(cap=7), want_of(r=np.inf)
    cands, wc, ncand = base(case.metric)[4], want[2].astype(np.int64), want[3]
    assert ((wc > 0) & (wc < ncand)).any() and (wc == 0).any() and ncand[-2] > 256  # fewer matches than candidates, none, the blob
    assert any(np.unique(cands[i][0][np.isin(cands[i][0], want[0][i, :wc[i]])], return_counts=True)[1].max(initial=0) > 1
               for i in range(len(q)))                           # a matching id sits in several selected lists
    assert (want7[2] > 7).any() and over[2][-1] == ref.U32_MAX and (over[2][:-1] != ref.U32_MAX).all() and over[2][:-1].any()
    tq = q if entry == "host" else torch.from_numpy(q).cuda()
    call(idx, tq, r, x, want=want)
    call(idx, tq, r, x, 7, want=want7)                           # counts run past the capacity, the padding is intact
    call(idx, tq, np.inf, x, want=over)                          # the far query is over the limit, the others still answer
    call(idx, tq, r, np.nan, want=want_of(x=np.nan))


@pytest.mark.parametrize("total", [1, 2, 37, ref.DISTINCT_MAX, ref.DISTINCT_MAX + 1])
def test_candidates_at_the_size_edges(main, total):
    """the last query has exactly `total` candidates at r: one, two, no power of two, the limit (answered) and one more
    (UINT32_MAX and an empty row); x = +inf keeps every scored id, so the dense list and the hit walk run at the same sizes"""
    case, q, idx, raw, r, x, want_of = main
    s = np.sort(base(case.metric)[4][-1][1])
    assert s[total - 1] < s[total]
    for xx in (np.inf, x):
        want = want_of(r=s[total], x=xx)
        assert (want[2][-1] == ref.U32_MAX) == (total > ref.DISTINCT_MAX) and (want[3][-1] >= 1 or total > ref.DISTINCT_MAX)
        call(idx, q, s[total], xx, want=want)


def test_rows_without_a_match_chunks_repeats_and_f16_queries(main):
    case, q, idx, raw, r, x, want_of = main
    want, bad = want_of(), case.x.copy()
    bad[int(want[0][np.nonzero(want[2])[0][0], 0]), 5] = np.nan  # a NaN in a row that matches
    try:
        for rows in (bad, case.x[:len(case.x) // 2]):            # ... and rows for half of the ids only
            got = want_of(rows=attach(idx, rows, raw))
            assert got[2].sum() < want[2].sum()
            call(idx, q, r, x, want=got)
    finally:
        attach(idx, case.x, raw)
    first, again = call(idx, q, r, x, want=want), call(idx, q, r, x)
    try:
        idx.set_option("mstg_search_budget", 1)                  # one query per chunk
        cut = call(idx, q, r, x)
    finally:
        idx.set_option("mstg_search_budget", 0)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(first, again, cut))
    q16 = q.astype(np.float16)
    assert all(np.array_equal(a, b) for a, b in zip(call(idx, q16.astype(np.float32), r, x), call(idx, q16, r, x)))


def test_refusals_and_binding(main):
    case, q, idx, raw, r, x, want_of = main
    for setup, undo, text in ((lambda: None, lambda: None, "distinct 1"), (lambda: idx.set_option("rerank", 0), lambda: idx.set_option("rerank", 1), "rerank 1"),
                              (lambda: idx.set_rerank_vectors(None), lambda: attach(idx, case.x, raw), "raw vectors attached")):
        setup()
        try:
            for tq in (q, torch.from_numpy(q).cuda()):
                with pytest.raises(rq.RabitqError, match=text) as e:
                    rq.mstg_range_rows(idx, tq, x, CAP, EF, EPS, text != "distinct 1", exact=True, candidate_radius=r)
                assert e.value.code == _abi.RBQ_INVALID_CONFIG and options(idx) == OFF
        finally:
            undo()
    (wi, wb, wc), (lims, ids, dist) = want_of()[:3], rq.mstg_range_search(idx, q, x, EF, EPS, exact=True, candidate_radius=r)
    assert np.array_equal(np.diff(lims), wc) and options(idx) == OFF
    for i in range(len(q)):
        assert np.array_equal(ids[lims[i]:lims[i + 1]], wi[i, :wc[i]]) and np.array_equal(dist[lims[i]:lims[i + 1]].view(np.uint32), wb[i, :wc[i]])
    with pytest.raises(rq.RabitqError, match="RBQ_MSTG_RANGE_DISTINCT_MAX"):
        rq.mstg_range_search(idx, q, x, EF, EPS, exact=True)    # candidate_radius None: +inf, the far query is over the limit
    m = rq.MstgIndex(64, "euclidean" if case.metric == 0 else "angular", default_ef_search=EF, pruning_epsilon=EPS)
    m.handle = idx
    assert [len(v) for v in m.range_query(q, x, exact=True, candidate_radius=r)] == wc.tolist()
