"""The exact range search on the GPU (options "range_exact" / "range_exact_radius_bits", k_range<..., XR, XIP> of k_range_exact.hip;
DESIGN.md section 33) against its restatement over the CPU oracle (tests/range_exact_ref.py): ids, exact score bits, totals and
padding are compared exactly, SearchDiagnostics where requested.  tests/test_range_exact_host.py shows on the CPU that the base
cases reject candidates and lose matches at a narrow candidate radius.  Run with `pytest -m gpu` on an MI355X."""
import functools

import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
import range_exact_ref as xref
import range_ref
import rerank_f16_ref
from conftest import make_dataset
from test_gpu_range import _bits, _case, _same, _words

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
NPROBE = 6


def _rounded(a, kind):
    """(what the library is handed, the f32 values it reads) for f32 data kept as `kind`"""
    if kind == "f32":
        return a, a
    h = rerank_f16_ref.round_to(a, kind)
    return (h.view(np.float16) if kind == "f16" else h), rerank_f16_ref.widen(h, kind)


def _open(built, rows, kind="f32", **kw):
    idx = rq.IvfRabitqIndex.from_built(built, **kw)
    idx.set_rerank_vectors(rows, dtype=kind)
    return idx


def _call(idx, q, x, r, cap, nprobe=NPROBE, fw=None, nbits=0, diag=True, dtype=None):
    idx.set_range_exact(x)
    idx.set_range_search(r)
    try:
        return idx.batch_search_raw(q, rq.SearchParams(cap, nprobe), fw, nbits, want_diag=diag, dtype=dtype)
    finally:
        idx.set_range_search(None)
        idx.set_range_exact(None)


def _cap(ref):
    return max(max(len(x[0]) for x in ref), 1) + 3


@functools.lru_cache(maxsize=None)
def _setup(metric, bits, dim, n=3000, raw_kind="f32", q_kind="f32"):
    """(data, built, rows handed over, queries handed over, widened rows, widened queries, x, [r at the estimate's 21st, 50th, unbounded])"""
    data, built, q = _case(metric, bits, dim, n)
    rows, wrows = _rounded(data, raw_kind)
    qs, wq = _rounded(q, q_kind)
    x = xref.kth_exact_score(built, wq[0], wrows, 21, NPROBE)
    radii = [range_ref.kth_distance_radius(built, wq[0], 21, NPROBE), range_ref.kth_distance_radius(built, wq[0], 50, NPROBE),
             xref.unbounded_radius(metric)]
    return data, built, rows, qs, wrows, wq, x, radii


@functools.lru_cache(maxsize=None)
def _ref(metric, bits, dim, n, raw_kind, q_kind, ri):
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim, n, raw_kind, q_kind)
    return xref.range_exact_batch(built, wq, wrows, x, radii[ri], NPROBE)


def _run(metric, bits, dim, n=3000, raw_kind="f32", q_kind="f32", ris=(0, 1, 2), diags=(True, False)):
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim, n, raw_kind, q_kind)
    qd = None if q_kind == "f32" else q_kind
    idx = _open(built, rows, raw_kind)
    try:
        for ri in ris:
            ref = _ref(metric, bits, dim, n, raw_kind, q_kind, ri)
            cap = _cap(ref)
            for diag in diags:
                _same(_call(idx, qs, x, radii[ri], cap, diag=diag, dtype=qd), ref, cap, diag, what=f"r {radii[ri]} x {x} diag {diag}")
        assert sum(len(e[0]) for e in ref) > 0
    finally:
        idx.close()


# ---- 1. base cases: both metrics, 1 / 3 / 7 bits, the three candidate radii, with and without SearchDiagnostics -------------------
@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_base(metric, bits):
    _run(metric, bits, 64)


# ---- 2. dimensions: 100 (padded to 128), 192, 33 (odd: 16-bit rows go element by element), 5 (the scalar tail alone), 960 ----------
@pytest.mark.parametrize("dim,raw_kind", [(100, "f32"), (192, "f32"), (33, "f32"), (33, "f16"), (33, "bf16"), (5, "f32"), (5, "f16")])
@pytest.mark.parametrize("bits", [1, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_dimensions(metric, bits, dim, raw_kind):
    _run(metric, bits, dim, raw_kind=raw_kind, ris=(0, 2), diags=(True,))


def test_dim_960():
    _run(0, 7, 960, n=2000, ris=(0, 2), diags=(True,))


# ---- 3. raw rows as f16 / bf16 (rounded here, the reference over the widened rows) and f32; a borrowed device pointer ---------------
@pytest.mark.parametrize("raw_kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_raw_dtypes(metric, raw_kind):
    _run(metric, 3, 64, raw_kind=raw_kind, ris=(0, 2), diags=(True,))


@pytest.mark.parametrize("raw_kind", ["f32", "f16"])
def test_borrowed_device_rows(raw_kind):
    """a torch tensor's pointer, and the same rows one element into an allocation: f32 rows off a 16-byte boundary, f16 rows of an
    even dimension at 2 mod 4 (the element path)"""
    import torch
    metric, bits, dim, n = 0, 3, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim, n, raw_kind)
    ref = _ref(metric, bits, dim, n, raw_kind, "f32", 2)
    cap = _cap(ref)
    dev = torch.device("cuda", 0)
    d_raw = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    d_off = torch.empty(rows.size + 1, dtype=d_raw.dtype, device=dev)
    d_off[1:] = d_raw.reshape(-1)
    torch.cuda.synchronize()
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for ptr in (d_raw.data_ptr(), d_off.data_ptr() + d_off.element_size()):
            idx.set_rerank_vectors(device_ptr=ptr, n=n, dtype=raw_kind)
            _same(_call(idx, qs, x, radii[2], cap), ref, cap, what=f"borrowed {raw_kind} rows at {ptr % 16} mod 16")
    finally:
        idx.close()


# ---- 4. 16-bit queries, alone and together with 16-bit rows ------------------------------------------------------------------------
@pytest.mark.parametrize("raw_kind,q_kind", [("f32", "f16"), ("f32", "bf16"), ("f16", "f16"), ("bf16", "bf16"), ("bf16", "f16")])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_query_dtypes(metric, raw_kind, q_kind):
    _run(metric, 3, 64, raw_kind=raw_kind, q_kind=q_kind, ris=(0, 2), diags=(True,))


# ---- 5. filter, with SearchDiagnostics (every candidate's filter bit is tested: no block skip) and without (block skip) -------------
def test_filter():
    metric, bits, dim, n = 0, 7, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    allowed = set(int(i) for i in np.nonzero(np.random.default_rng(3400).random(n) < 0.3)[0])
    idx = _open(built, rows)
    try:
        for nbits, keep in ((n, allowed), (n // 2, set(i for i in allowed if i < n // 2))):
            fw = _words(keep, nbits)
            for r in radii[1:]:
                ref = xref.range_exact_batch(built, wq, wrows, x, r, NPROBE, keep)
                cap = _cap(ref)
                for diag in (True, False):
                    _same(_call(idx, qs, x, r, cap, fw=fw, nbits=nbits, diag=diag), ref, cap, diag, what=f"filter {nbits} bits, r {r}, diag {diag}")
            assert 0 < sum(len(e[0]) for e in ref) < sum(len(e[0]) for e in _ref(metric, bits, dim, n, "f32", "f32", 2))
    finally:
        idx.close()


# ---- 6. capacities -----------------------------------------------------------------------------------------------------------------
def test_capacities():
    """the totals do not depend on the capacity, a row is the uncapped result's prefix, the rest is padding; top_k 0 reports nothing"""
    metric, bits, dim, n = 0, 1, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    x = xref.kth_exact_score(built, wq[0], wrows, 60, NPROBE)  # (wider than the base x: totals of several tens)
    ref = xref.range_exact_batch(built, wq, wrows, x, radii[2], NPROBE)
    tot = [len(e[0]) for e in ref]
    T = max(tot)
    assert T > 40 and min(tot) == 0 and sum(t > 7 for t in tot) > 1
    idx = _open(built, rows)
    try:
        for cap in (T + 5, T, 1, 7, T - 1):
            _same(_call(idx, qs, x, radii[2], cap), ref, cap, what=f"cap {cap}")
        idx.set_range_exact(x)
        idx.set_range_search(radii[2])
        ids, sc, cnt, dg = idx.batch_search_raw(qs, rq.SearchParams(0, NPROBE), want_diag=True)
        assert not cnt.any() and not dg.any()
    finally:
        idx.close()


# ---- 7. raw rows for the first half of the ids only ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_ids_without_a_raw_row_never_match(metric):
    bits, dim, n = 3, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    full = _ref(metric, bits, dim, n, "f32", "f32", 2)
    ref = xref.range_exact_batch(built, wq, wrows[:n // 2], x, radii[2], NPROBE)
    assert sum(len(e[0]) for e in ref) < sum(len(e[0]) for e in full) and all((e[0] < n // 2).all() for e in ref)
    idx = _open(built, rows[:n // 2])
    try:
        cap = _cap(full)
        got = _call(idx, qs, x, radii[2], cap)
        _same(got, ref, cap, what="half of the rows attached")
        assert (got[0][got[0] != range_ref.PAD_ID] < n // 2).all()
    finally:
        idx.close()


# ---- 8. the device entry on a side stream ---------------------------------------------------------------------------------------------
def test_device_entry():
    import torch
    metric, bits, dim, n = 0, 7, 100, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    ref = _ref(metric, bits, dim, n, "f32", "f32", 1)
    cap = _cap(ref)
    nq = len(qs)
    idx = _open(built, rows)
    try:
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(qs).to(dev)
        d_i = torch.zeros(nq, cap, dtype=torch.int64, device=dev)
        d_s = torch.zeros(nq, cap, dtype=torch.float32, device=dev)
        d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_d = torch.zeros(nq, 3, dtype=torch.int64, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        idx.range_search_device(qd.data_ptr(), nq, dim, x, NPROBE, cap, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(),
                                stream=st.cuda_stream, d_diag=d_d.data_ptr(), exact=True, candidate_radius=radii[1])
        torch.cuda.synchronize(dev)
        idx.release_stream(st.cuda_stream)
        _same((d_i.cpu().numpy().view(np.uint64), d_s.cpu().numpy(), d_c.cpu().numpy().view(np.uint32), d_d.cpu().numpy().view(np.uint64)),
              ref, cap, what="device entry")
        # the stage probe while the options are on (nothing is launched): the exact kernel — 256 threads, no scratch, its larger LDS
        idx.set_range_search(radii[1])
        idx.set_option("rerank", 0)  # (the estimate-only range search is refused with the rerank on)
        plain = idx.stage_resources(nq, cap, NPROBE)["scan"]
        idx.set_option("rerank", 1)
        idx.set_range_exact(x)
        res = idx.stage_resources(nq, cap, NPROBE)["scan"]
        assert res["workgroups"] == nq and res["threads"] == 256 and res["scratch_bytes"] == 0, res
        assert res["lds_bytes"] == plain["lds_bytes"] + 256 * 12 + 16 + 4 * dim, (res, plain)
    finally:
        idx.close()


# ---- 9. numeric variants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [3, 7])
@pytest.mark.parametrize("variant,mask", [("native_avx2", 1), ("portable", 6)])
def test_numeric_variants(variant, mask, bits):
    metric, dim = (1 if bits == 3 else 0), 192
    data, built, q = _case(metric, bits, dim)
    idx = _open(built, data)
    try:
        idx.set_numeric_variant(variant)
        with oracle.variant(mask):
            x = xref.kth_exact_score(built, q[0], data, 21, NPROBE)
            for r in (range_ref.kth_distance_radius(built, q[0], 21, NPROBE), xref.unbounded_radius(metric)):
                ref = xref.range_exact_batch(built, q, data, x, r, NPROBE)
                cap = _cap(ref)
                _same(_call(idx, q, x, r, cap), ref, cap, what=f"{variant} r {r}")
            assert sum(len(e[0]) for e in ref) > 0
    finally:
        idx.close()


# ---- 10. non-finite input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_non_finite(metric):
    bits, dim, n = 7, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    full = _ref(metric, bits, dim, n, "f32", "f32", 2)
    victim = int(full[0][0][3])  # a match of query 0
    bad = data.copy()
    bad[victim, 17] = np.nan  # (inside the spans: an accumulator's chain) — the row's score is NaN for every query
    q = qs.copy()
    q[2, 5] = INF
    q[4, 63] = np.nan
    ref = xref.range_exact_batch(built, q, bad, x, radii[2], NPROBE)
    assert victim not in ref[0][0] and len(ref[0][0]) == len(full[0][0]) - 1
    assert len(ref[2][0]) == 0 and len(ref[4][0]) == 0
    idx = _open(built, bad)
    try:
        cap = _cap(ref)
        _same(_call(idx, q, x, radii[2], cap), ref, cap, what="NaN in a raw row, inf and NaN in queries")
        # a NaN x matches nothing, and the candidate scan's diagnostics stay
        nan = xref.range_exact_batch(built, q, bad, F32(np.nan), radii[2], NPROBE)
        assert all(len(e[0]) == 0 for e in nan)
        _same(_call(idx, q, F32(np.nan), radii[2], 4), nan, 4, what="NaN x")
    finally:
        idx.close()


# ---- 11. a host call of several sub-batches; the same call twice -----------------------------------------------------------------------
def test_many_queries_and_determinism():
    metric, bits, dim, n = 0, 3, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    ref = _ref(metric, bits, dim, n, "f32", "f32", 1)
    cap = _cap(ref)
    reps = 1500 // len(qs) + 1
    big = np.ascontiguousarray(np.tile(qs, (reps, 1))[:1500])
    big_ref = (ref * reps)[:1500]
    idx = _open(built, rows)
    two = _open(built, rows, devices=[0, 0])
    try:
        first = _call(idx, big, x, radii[1], cap)
        _same(first, big_ref, cap, what="1500 queries")
        again = _call(idx, big, x, radii[1], cap)
        for a, b in zip(first, again):
            assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)
        assert two.device_count() == 2
        _same(_call(two, big, x, radii[1], cap), big_ref, cap, what="two replicas")
    finally:
        idx.close()
        two.close()


# ---- 12. refusals and neutrality ---------------------------------------------------------------------------------------------------------
def _equal(a, b):
    return all(np.array_equal(_bits(u) if u.dtype == np.float32 else u, _bits(v) if v.dtype == np.float32 else v) for u, v in zip(a, b))


def test_refusals_and_neutrality():
    metric, bits, dim, n = 0, 7, 100, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    ref = _ref(metric, bits, dim, n, "f32", "f32", 1)
    cap = _cap(ref)
    P = rq.SearchParams(10, NPROBE)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        plain = idx.batch_search_raw(qs, P, want_diag=True)
        # range_exact 1 without vectors: refused, with a detail
        with pytest.raises(rq.RabitqError, match="raw vectors") as e:
            _call(idx, qs, x, radii[1], cap)
        assert e.value.kind == "InvalidConfig" and e.value.detail
        idx.set_rerank_vectors(rows)
        reranked = idx.batch_search_raw(qs, P, want_diag=True)
        idx.set_rerank_pool(64)
        pooled = idx.batch_search_raw(qs, P, want_diag=True)
        idx.set_rerank_pool(0)
        assert not _equal(plain[:2], reranked[:2])
        # range_exact 1 with the option rerank 0: refused
        idx.set_option("rerank", 0)
        with pytest.raises(rq.RabitqError, match="rerank") as e:
            _call(idx, qs, x, radii[1], cap)
        assert e.value.kind == "InvalidConfig" and e.value.detail
        idx.set_option("rerank", 1)
        # range_exact 0 with the rerank on: the old refusal, text unchanged
        idx.set_range_search(radii[1])
        with pytest.raises(rq.RabitqError) as e:
            idx.batch_search_raw(qs, rq.SearchParams(cap, NPROBE))
        assert e.value.kind == "InvalidConfig"
        assert e.value.detail == "range search does not run with the rerank on: set the option rerank 0 or detach the vectors"
        idx.set_range_search(None)
        # rerank_pool is not read in range mode
        want = _call(idx, qs, x, radii[1], cap)
        _same(want, ref, cap, what="exact call")
        idx.set_rerank_pool(64)
        assert _equal(_call(idx, qs, x, radii[1], cap), want)
        idx.set_rerank_pool(0)
        # range_exact alone (range_search 0) changes nothing: the reranked and the pooled top-k search, bit for bit
        idx.set_range_exact(x)
        assert _equal(idx.batch_search_raw(qs, P, want_diag=True), reranked)
        idx.set_rerank_pool(64)
        assert _equal(idx.batch_search_raw(qs, P, want_diag=True), pooled)
        idx.set_rerank_pool(0)
        idx.set_range_exact(None)
        # every option off again: the three searches answer as before
        assert _equal(idx.batch_search_raw(qs, P, want_diag=True), reranked)
        idx.set_rerank_pool(64)
        assert _equal(idx.batch_search_raw(qs, P, want_diag=True), pooled)
        idx.set_rerank_pool(0)
        idx.set_option("rerank", 0)
        assert _equal(idx.batch_search_raw(qs, P, want_diag=True), plain)
        # and the estimate-only range search runs as ever with the rerank off
        est = range_ref.range_batch(built, qs, radii[1], NPROBE)
        idx.set_range_search(radii[1])
        _same(idx.batch_search_raw(qs, rq.SearchParams(_cap(est), NPROBE), want_diag=True), est, _cap(est), what="estimate-only")
        idx.set_range_search(None)
    finally:
        idx.close()


# ---- 13. the FAISS-style wrapper ---------------------------------------------------------------------------------------------------------
def test_wrapper():
    metric, bits, dim, n = 0, 7, 64, 3000
    data, built, rows, qs, wrows, wq, x, radii = _setup(metric, bits, dim)
    nlist = built.n_lists
    idx = _open(built, rows)
    try:
        ref = _ref(metric, bits, dim, n, "f32", "f32", 1)
        lims, ids, sc = idx.range_search(qs, x, NPROBE, exact=True, candidate_radius=radii[1])
        assert np.array_equal(np.diff(lims), [len(e[0]) for e in ref])
        assert np.array_equal(ids, np.concatenate([e[0] for e in ref])) and np.array_equal(_bits(sc), _bits(np.concatenate([e[1] for e in ref])))
        # candidate_radius=None: unbounded by metric
        ref = _ref(metric, bits, dim, n, "f32", "f32", 2)
        lims, ids, sc, dg = idx.range_search(qs, x, NPROBE, exact=True, want_diag=True)
        assert np.array_equal(np.diff(lims), [len(e[0]) for e in ref]) and np.array_equal(ids, np.concatenate([e[0] for e in ref]))
        assert np.array_equal(dg, xref.diag_of(ref))
        # infinite x and r over every list: more than 1024 matches per query, the repeat call
        every = xref.range_exact_batch(built, wq[:3], wrows, INF, INF, nlist)
        assert min(len(e[0]) for e in every) > 1024
        lims, ids, sc = idx.range_search(qs[:3], INF, nlist, exact=True)
        assert np.array_equal(np.diff(lims), [len(e[0]) for e in every])
        assert np.array_equal(ids, np.concatenate([e[0] for e in every])) and np.array_equal(_bits(sc), _bits(np.concatenate([e[1] for e in every])))
        lims, ids, sc, tot, dg = idx.range_search(qs[:3], INF, nlist, max_results=100, want_diag=True, sort=True, exact=True)
        assert np.array_equal(tot, [len(e[0]) for e in every]) and np.array_equal(lims, [0, 100, 200, 300])
        assert np.array_equal(dg, xref.diag_of(every))
        for i, (rid, rsc, _) in enumerate(every):
            o = np.argsort(rsc[:100], kind="stable")
            assert np.array_equal(ids[lims[i]:lims[i + 1]], rid[:100][o])
            assert np.array_equal(_bits(sc[lims[i]:lims[i + 1]]), _bits(rsc[:100][o]))
        keep = set(range(0, n, 2))
        part = xref.range_exact_batch(built, wq, wrows, x, radii[2], NPROBE, keep)
        lims, ids, sc = idx.range_search(qs, x, NPROBE, allowed_ids=range(0, n, 2), exact=True)
        assert np.array_equal(np.diff(lims), [len(e[0]) for e in part]) and np.array_equal(ids, np.concatenate([e[0] for e in part]))
        # the options are put back: the reranked top-k search answers as before
        before = idx.batch_search_raw(qs, rq.SearchParams(10, NPROBE))
        idx.range_search(qs, x, NPROBE, exact=True)
        assert _equal(idx.batch_search_raw(qs, rq.SearchParams(10, NPROBE))[:3], before[:3])
        with pytest.raises(rq.RabitqError):
            idx.range_search(qs, x, NPROBE, candidate_radius=radii[1])  # (candidate_radius goes with exact=True)
    finally:
        idx.close()
