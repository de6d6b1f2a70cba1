"""Range search on the GPU (options "range_search" / "range_radius_bits", k_range) against its restatement
over the CPU oracle (tests/range_ref.py): ids, score bits, totals and padding are compared exactly, SearchDiagnostics where
requested.  Run with `pytest -m gpu` on an MI355X."""
import functools

import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
import range_ref
from conftest import build_index, make_dataset

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _queries(data, dim, nlist, metric, seed, nq=8):
    """nq - 1 generator queries and one that is far from everything (no match at any radius taken from query 0)"""
    q = make_dataset(nq - 1, dim, max(nlist // 4, 1), seed, normalize=(metric == 1))
    far = (data.mean(0) + F32(25.0)) if metric == 0 else F32(0.01) * q[1]  # (a short query: every score is a hundredth of a usual one)
    return np.ascontiguousarray(np.concatenate([q, far[None, :]]), dtype=F32)


@functools.lru_cache(maxsize=None)
def _case(metric, bits, dim, n=3000, nlist=12, seed=3100):
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, normalize=(metric == 1), seed=seed + dim + bits)
    return data, built, _queries(data, dim, nlist, metric, seed + 7 + dim)


def _radii(built, q, nprobe, ks=(6, 21, 50)):
    """the caller's radius at query 0's 6th / 21st / 50th top-k distance: query 0 gets 5 / 20 / 49 matches"""
    return [range_ref.kth_distance_radius(built, q[0], k, nprobe) for k in ks]


def _exercised(refs):
    """The reference results of a case must exercise the kernel: a query without a match, one with more than a half-wave's worth,
    and vectors on every branch — skipped by the bound, refined and rejected, matched."""
    tot = np.array([[len(r[0]) for r in ref] for ref in refs])
    dg = np.stack([range_ref.diag_of(ref) for ref in refs]).astype(np.int64)
    assert (tot == 0).any(), "no query without a match"
    assert (tot > 32).any(), "no query with more than 32 matches"
    assert dg[..., 1].sum() > 0, "nothing skipped by the lower bound"
    assert (dg[..., 0].sum(axis=-1) - tot.sum(axis=-1) > 0).all(), "nothing refined and rejected"
    assert tot.sum() > 0, "nothing matched"


def _call(idx, q, radius, nprobe, cap, fw=None, nbits=0, diag=True):
    idx.set_range_search(radius)
    try:
        return idx.batch_search_raw(q, rq.SearchParams(cap, nprobe), fw, nbits, want_diag=diag)
    finally:
        idx.set_range_search(None)


def _same(got, ref, cap, diag=True, what=""):
    ids, sc, cnt, dg = got
    eids, ebits, etot = range_ref.rows(ref, cap)
    assert np.array_equal(cnt, etot), f"{what}: totals {cnt} expected {etot}"
    bad = np.nonzero((ids != eids).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8]}: gpu={ids[bad[0]][:12]} expected={eids[bad[0]][:12]}"
    sbad = np.nonzero((_bits(sc) != ebits).any(axis=1))[0]
    assert sbad.size == 0, f"{what}: score bits differ for queries {sbad[:8]}"
    if diag:
        assert np.array_equal(dg, range_ref.diag_of(ref)), f"{what}: SearchDiagnostics {dg.tolist()} expected {range_ref.diag_of(ref).tolist()}"


def _check(idx, built, q, radius, nprobe, cap=None, allowed=None, fw=None, nbits=0, diag=True, what=""):
    ref = range_ref.range_batch(built, q, radius, nprobe, allowed)
    cap = cap or max(max(len(r[0]) for r in ref), 1) + 3
    _same(_call(idx, q, radius, nprobe, cap, fw, nbits, diag), ref, cap, diag, what)
    return ref


def _words(allowed, nbits):
    w = np.zeros((nbits + 31) // 32 or 1, np.uint32)
    a = np.array([i for i in allowed if i < nbits], np.uint64)
    np.bitwise_or.at(w, (a >> np.uint64(5)).astype(np.int64), (np.uint32(1) << (a & np.uint64(31)).astype(np.uint32)))
    return w


# ---- 1. base shape: both metrics, 1 / 3 / 7 bits; dim 64 (tail-only granule), 100 (FHT padding to 128: the compile-time 128
# kernel), 192 (a granule plus the tail at runtime dimension); one 7-bit case at dim 960 -------------------------------------------
def _base_refs(metric, bits, dim, n, nprobe=6):
    data, built, q = _case(metric, bits, dim, n)
    radii = _radii(built, q, nprobe)
    refs = [range_ref.range_batch(built, q, r, nprobe) for r in radii]
    # query 0 gets the k - 1 results nearer than its k-th: 5 / 20 / 49 (one or two fewer where two distances are equal)
    assert all(k - 3 <= len(ref[0][0]) <= k - 1 for k, ref in zip((6, 21, 50), refs)), [len(ref[0][0]) for ref in refs]
    _exercised(refs)
    return built, q, radii, refs


def _base(metric, bits, dim, n, range_kernel=False):
    nprobe = 6
    built, q, radii, refs = _base_refs(metric, bits, dim, n, nprobe)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for r, ref in zip(radii, refs):
            cap = max(len(x[0]) for x in ref) + 3
            if range_kernel:  # the stage probe while the option is on (nothing is launched): k_range — 256 threads, no scratch
                assert built.padded_dim == dim
                idx.set_range_search(r)
                try:
                    res = idx.stage_resources(len(q), cap, nprobe)["scan"]
                finally:
                    idx.set_range_search(None)
                assert res["workgroups"] == len(q) and res["threads"] == 256 and res["scratch_bytes"] == 0, res
            _same(_call(idx, q, r, nprobe, cap), ref, cap, what=f"radius {r}")
            _same(_call(idx, q, r, nprobe, cap, diag=False), ref, cap, diag=False, what=f"radius {r}, no diagnostics")
    finally:
        idx.close()


@pytest.mark.parametrize("dim", [64, 100, 192])
@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_base_shape(metric, bits, dim):
    _base(metric, bits, dim, 3000)


def test_dim_960():
    _base(0, 7, 960, 2000)


# the other compile-time instantiations, k_range<768, *> and k_range<960, 0 / 2> (k_range.hip: launch_range_d), and that it is
# k_range the stage probe reports for them
@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_dim_768(metric, bits):
    _base(metric, bits, 768, 2000, range_kernel=True)


@pytest.mark.parametrize("bits", [1, 3])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_dim_960_one_and_three_bits(metric, bits):
    _base(metric, bits, 960, 2000, range_kernel=True)


# ---- 2. capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity():
    """the totals do not depend on the capacity, the head is the uncapped result's prefix, the tail is padding"""
    data, built, q = _case(0, 7, 64)
    nprobe = 6
    r = _radii(built, q, nprobe)[2]
    ref = range_ref.range_batch(built, q, r, nprobe)
    T = len(ref[0][0])
    assert T == 49
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for cap in (1, T - 1, T, T + 1):
            _same(_call(idx, q, r, nprobe, cap), ref, cap, what=f"cap {cap}")
        wide = range_ref.range_batch(built, q, INF, nprobe)  # every query has matches: a capacity below every total
        low = min(len(x[0]) for x in wide)
        assert low > 40
        _same(_call(idx, q, INF, nprobe, 40), wide, 40, what="cap below every total")
    finally:
        idx.close()


# ---- 3. radius edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_radius_edges(metric):
    data, built, q = _case(metric, 7, 64)
    nprobe = 6
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        nan = _check(idx, built, q, F32(np.nan), nprobe, what="NaN")  # keeps and skips nothing
        assert all(len(x[0]) == 0 and x[2][1] == 0 and x[2][2] > 0 for x in nan)
        none = _check(idx, built, q, -INF if metric == 0 else INF, nprobe, what="the empty radius")
        assert all(len(x[0]) == 0 for x in none)
        # the radius that admits every finite distance, at a capacity of at least the probed vectors: as a set, what the top-k
        # search returns at top_k = cap with the option off
        cap = len(data)
        everything = _check(idx, built, q, INF if metric == 0 else -INF, nprobe, cap=cap, what="the unbounded radius")
        ids, sc, cnt, _ = idx.batch_search_raw(q, rq.SearchParams(cap, nprobe))
        for i, (rid, rsc, _) in enumerate(everything):
            c = int(cnt[i])
            assert c == len(rid) > 0
            a, b = np.lexsort((_bits(rsc), rid)), np.lexsort((_bits(sc[i, :c]), ids[i, :c]))
            assert np.array_equal(rid[a], ids[i, :c][b]) and np.array_equal(_bits(rsc)[a], _bits(sc[i, :c])[b])
        # a radius equal to a stored match's score excludes it; the next f32 on the admitting side includes it
        mid, msc, _ = range_ref.range_batch(built, q, _radii(built, q, nprobe)[1], nprobe)[0]
        s = F32(msc[7])
        at = _check(idx, built, q, s, nprobe, what="radius = a match's score")
        nxt = _check(idx, built, q, np.nextafter(s, INF if metric == 0 else -INF), nprobe, what="the next radius")
        assert mid[7] not in at[0][0] and mid[7] in nxt[0][0]
    finally:
        idx.close()


# ---- 4. list shapes: an empty list among the probed, lists of 1 / 31 / 32 / 33 vectors, nprobe above the number of lists ---------
SIZES = [0, 1, 31, 32, 33, 300, 0, 65]


@pytest.mark.parametrize("bits", [1, 7])
def test_list_shapes(bits):
    rng = np.random.default_rng(3300)
    n = sum(SIZES)
    data = make_dataset(n, 64, 4, 3301)
    assign = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES)).astype(np.uint32)
    cent = np.stack([data[assign == c].mean(0) if s else data[c] for c, s in enumerate(SIZES)]).astype(F32)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, 0, 1, 3302, True)
    q = np.ascontiguousarray(np.concatenate([data[[5, 77, 300]] + F32(0.01), cent[[0, 1, 6]]]), dtype=F32)  # (at the empty lists' centroids too)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        radii = _radii(built, q, len(SIZES), ks=(4, 30)) + [INF]
        for nprobe in (len(SIZES), len(SIZES) + 3, 3):
            for r in radii:
                ref = _check(idx, built, q, r, nprobe, what=f"nprobe {nprobe} radius {r}")
        assert sum(len(x[0]) for x in ref) > 0
    finally:
        idx.close()
        built.close()


# ---- 5. filter --------------------------------------------------------------------------------------------------------------------
def test_filter():
    """about 30 % of the ids, with diagnostics (every candidate's filter bit is tested: no block skip) and without (block skip);
    and a filter shorter than the id space"""
    data, built, q = _case(0, 7, 64)
    n, nprobe = len(data), 6
    rng = np.random.default_rng(3400)
    allowed = set(int(i) for i in np.nonzero(rng.random(n) < 0.3)[0])
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for nbits, keep in ((n, allowed), (n // 2, set(i for i in allowed if i < n // 2))):
            fw = _words(keep, nbits)
            for r in _radii(built, q, nprobe)[1:] + [INF]:
                ref = range_ref.range_batch(built, q, r, nprobe, keep)
                cap = max(max(len(x[0]) for x in ref), 1) + 2
                _same(_call(idx, q, r, nprobe, cap, fw, nbits, diag=True), ref, cap, what=f"filter {nbits} bits, radius {r}")
                _same(_call(idx, q, r, nprobe, cap, fw, nbits, diag=False), ref, cap, diag=False, what=f"filter {nbits} bits, radius {r}, no diagnostics")
            assert sum(len(x[0]) for x in ref) > 0
    finally:
        idx.close()


# ---- 6. numeric variants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [3, 7])
@pytest.mark.parametrize("variant,mask", [("native_avx2", 1), ("portable", 6)])
def test_numeric_variants(variant, mask, bits):
    data, built, q = _case(1 if bits == 3 else 0, bits, 192)
    nprobe = 6
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        idx.set_numeric_variant(variant)
        with oracle.variant(mask):
            for r in _radii(built, q, nprobe):
                _check(idx, built, q, r, nprobe, what=f"{variant} radius {r}")
    finally:
        idx.close()


# ---- 7. entries -------------------------------------------------------------------------------------------------------------------
def test_entries():
    import torch
    data, built, q = _case(0, 7, 100)
    nq, dim, nprobe = len(q), q.shape[1], 6
    r = _radii(built, q, nprobe)[2]
    ref = range_ref.range_batch(built, q, r, nprobe)
    cap = max(len(x[0]) for x in ref) + 1
    idx = rq.IvfRabitqIndex.from_built(built)
    two = rq.IvfRabitqIndex.from_built(built, devices=[0, 0])
    try:
        _same(_call(idx, q, r, nprobe, cap), ref, cap, what="host entry")
        _same(_call(idx, q[:1], r, nprobe, cap), ref[:1], cap, what="one query")
        idx.set_option("host_subbatch", 3)  # 8 queries in sub-batches of at most 3
        _same(_call(idx, q, r, nprobe, cap), ref, cap, what="three sub-batches")
        idx.set_option("host_subbatch", 0)
        assert two.device_count() == 2
        _same(_call(two, q, r, nprobe, cap), ref, cap, what="two replicas")
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(q).to(dev)
        d_i = torch.zeros(nq, cap, dtype=torch.int64, device=dev)
        d_s = torch.zeros(nq, cap, dtype=torch.float32, device=dev)
        d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_d = torch.zeros(nq, 3, dtype=torch.int64, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        idx.range_search_device(qd.data_ptr(), nq, dim, r, nprobe, cap, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(),
                                stream=st.cuda_stream, d_diag=d_d.data_ptr())
        torch.cuda.synchronize(dev)
        idx.release_stream(st.cuda_stream)
        _same((d_i.cpu().numpy().view(np.uint64), d_s.cpu().numpy(), d_c.cpu().numpy().view(np.uint32), d_d.cpu().numpy().view(np.uint64)),
              ref, cap, what="device entry")
    finally:
        idx.close()
        two.close()


# ---- 8. options and refusals ------------------------------------------------------------------------------------------------------
def test_options_and_refusals():
    data, built, q = _case(0, 7, 100)
    nprobe = 6
    r = _radii(built, q, nprobe)[2]
    ref = range_ref.range_batch(built, q, r, nprobe)
    cap = max(len(x[0]) for x in ref) + 1
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        before = idx.batch_search_raw(q, rq.SearchParams(10, nprobe), want_diag=True)  # (the option has never been set)
        for opt, on, off in (("block_bound", 0, 1), ("exact_rank", 1, 0), ("force_rank_fallback", 1, 0)):
            idx.set_option(opt, on)
            _same(_call(idx, q, r, nprobe, cap), ref, cap, what=f"{opt} {on}")
            idx.set_option(opt, off)
        # the rerank on: refused, with a detail
        idx.set_rerank_vectors(data)
        with pytest.raises(rq.RabitqError, match="range search") as e:
            _call(idx, q, r, nprobe, cap)
        assert e.value.kind == "InvalidConfig" and e.value.detail
        idx.set_rerank_vectors(None)
        # top_k = 0: no match is reported
        idx.set_range_search(r)
        ids, sc, cnt, dg = idx.batch_search_raw(q, rq.SearchParams(0, nprobe), want_diag=True)
        assert not cnt.any() and not dg.any()
        idx.set_range_search(None)
        # with the option off again the handle answers the top-k search as it did before, bit for bit
        after = idx.batch_search_raw(q, rq.SearchParams(10, nprobe), want_diag=True)
        for a, b in zip(before, after):
            assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)
    finally:
        idx.close()


# ---- 9. the FAISS-style wrapper ---------------------------------------------------------------------------------------------------
def test_wrapper():
    data, built, q = _case(0, 7, 64)
    nlist = built.n_lists
    ref = range_ref.range_batch(built, q[:3], INF, nlist)  # every vector of the index: the first call's rows of 1024 truncate
    assert min(len(x[0]) for x in ref) > 1024
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        lims, ids, sc = idx.range_search(q[:3], INF, nlist)
        assert np.array_equal(np.diff(lims), [len(x[0]) for x in ref])
        assert np.array_equal(ids, np.concatenate([x[0] for x in ref]))
        assert np.array_equal(_bits(sc), _bits(np.concatenate([x[1] for x in ref])))
        lims, ids, sc, tot, dg = idx.range_search(q[:3], INF, nlist, max_results=100, want_diag=True, sort=True)
        assert np.array_equal(tot, [len(x[0]) for x in ref]) and np.array_equal(lims, [0, 100, 200, 300])
        assert np.array_equal(dg, range_ref.diag_of(ref))
        for i, (rid, rsc, _) in enumerate(ref):
            o = np.argsort(rsc[:100], kind="stable")
            assert np.array_equal(ids[lims[i]:lims[i + 1]], rid[:100][o])
            assert np.array_equal(_bits(sc[lims[i]:lims[i + 1]]), _bits(rsc[:100][o]))
        r = _radii(built, q, 6)[1]
        part = range_ref.range_batch(built, q, r, 6, set(range(0, len(data), 2)))
        lims, ids, sc = idx.range_search(q, r, 6, allowed_ids=range(0, len(data), 2))
        assert np.array_equal(np.diff(lims), [len(x[0]) for x in part]) and np.array_equal(ids, np.concatenate([x[0] for x in part]))
        # the options are put back: the top-k search answers as ever
        rc, oids, osc, ocnt, _ = oracle.search_batch(built, q, 10, 6)
        gids, gsc, gcnt, _ = idx.batch_search_raw(q, rq.SearchParams(10, 6))
        assert rc == 0 and np.array_equal(gids, oids) and np.array_equal(gcnt, ocnt)
    finally:
        idx.close()
