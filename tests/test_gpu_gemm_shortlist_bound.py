"""The GEMM-shortlist front end (k_gemm_shortlist.hip) against the float64 bounds its scans rely on, and the five paths behind it
on near-ties at the scale of eps.

k-means assignment, the hierarchical splits, IvfRabitqIndex.add's nearest list, the MSTG closure assignment and the MSTG list
selection all shortlist {c : A(c) <= threshold + 2.01 eps} from the front's approximate distances A and score only the shortlist
exactly, so each is exact only while |A - canonical| <= eps.  Their other tests compare final results on data whose nearest
centroids are many eps apart, which a front end that is slightly wrong would pass.  Here

  * the tap rbq_debug_gemm_shortlist_front gives the front's own outputs, and every (row, centroid) pair is held to: the split
    images and the norms bit for bit, the raw dots to the ranking GEMM's float64 budget (rank_bound.check_rows), and |A - C| <= eps
    for k_km_scan's (canonical form, eps) and for the closure / selection one (tests/gemm_shortlist_bound.py); at one slab and at
    79, ragged in rows and centroids, over several passes, and over magnitudes from 1e-20 to 1e18;
  * seeded near-ties (tests/neartie_cases.py: the gap between the two nearest centroids uniform in [-4 eps, 4 eps]) go through
    IvfRabitqIndex.add, closure_assign and mstg_search end to end, with no row falling back, and must equal the CPU restatements;
    the closure's shortlist tap must hold exactly {c : A(c) <= T + 2.01 eps} for the A of the front-end tap, which is what pins
    the eps constant the kernels use (a library built with both eps 64 times too small passed every other test here: the
    front's error is at most 0.17 eps, so results alone do not show an eps that is too small).

Run with -s to see the worst error / budget per route (recorded in profiles/gemm_shortlist/bound_ratios.txt)."""
import numpy as np
import pytest

import gemm_shortlist_bound as gb
import kmeans_ref
import mstg_search_cases as mc
import neartie_cases as nt
import rabitq_rs_amd as rq
from rabitq_rs_amd import kmeans as rk
from rabitq_rs_amd import mstg
from rabitq_rs_amd.index import lib
from test_gpu_rank_bound import _data

pytestmark = pytest.mark.gpu

f32 = np.float32
# (n, k, dim, rows per pass or 0): one slab .. 79 slabs, ragged row and centroid tiles, one row, several passes
SHAPES = [(1, 1, 1, 0), (5, 257, 7, 0), (33, 300, 9, 0), (129, 257, 33, 0), (130, 513, 65, 0), (127, 260, 129, 0),
          (257, 1000, 100, 0), (64, 300, 960, 0), (3, 260, 2048, 0), (9, 260, 2500, 0), (300, 257, 64, 128)]
BUDGET_KINDS = ["mix_1e-4", "mix_1e4", "int255", "coord_scales", "offset"]  # dots and eps
EPS_ONLY = {"mix_1e-20": 1e-20, "mix_1e18": 1e18}                            # eps alone: its 2^-100 floor, spans near overflow
_WORST = {}  # route -> largest error / budget seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nGEMM-shortlist front: largest error / budget per route")
    for route in sorted(_WORST):
        print(f"  {route:<44s} {_WORST[route]:.4f}")


def _note(route, ratio):
    _WORST[route] = max(_WORST.get(route, 0.0), ratio)


def _operands(kind, n, k, dim, seed):
    if kind in EPS_ONLY:
        z = (_data("mix", n + k, dim, seed) * f32(EPS_ONLY[kind])).astype(f32)
    else:
        z = _data(kind, n + k, dim, seed)
    return np.ascontiguousarray(z[:n]), np.ascontiguousarray(z[n:])


def _tap(c, x, cap):
    L = lib()
    prev = L.rbq_debug_set_kmeans_chunk_rows(cap)
    try:
        return rk.debug_gemm_shortlist_front(c, x)
    finally:
        L.rbq_debug_set_kmeans_chunk_rows(prev)


@pytest.mark.parametrize("kind", BUDGET_KINDS + sorted(EPS_ONLY))
@pytest.mark.parametrize("n,k,dim,cap", SHAPES, ids=lambda v: str(v))
def test_front_end_within_its_bounds(n, k, dim, cap, kind):
    x, c = _operands(kind, n, k, dim, 5000 + 3 * n + 7 * k + dim)
    t = _tap(c, x, cap)
    tag = f"{kind} ({n}, {k}, {dim})"
    # (a) the split images, bit for bit, zeros beyond dim
    for name, src in (("row", x), ("cent", c)):
        hi, lo = gb.split_images(src)
        bad = np.nonzero((t[name + "_hi"] != hi).any(1) | (t[name + "_lo"] != lo).any(1))[0]
        assert bad.size == 0, f"{tag}: {name}_hi / {name}_lo differ from bf16_split, zero-padded, in rows {bad[:10]}"
    # (b) the canonical norms, bit for bit
    nx, nc = gb.km_norm(x), gb.km_norm(c)
    for name, got, want in (("nx", t["nx"], nx), ("nc", t["nc"], nc), ("ncmax", np.array([t["ncmax"]], f32), nc.max(keepdims=True))):
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, f"{tag}: {name} differs from km_norm at {bad[:10]}"
    # (c) the raw dots against the GEMM's float64 budget
    if kind not in EPS_ONLY:
        worst, viol = gb.check_dots(t["dots"], x, c)
        _note("dots / GEMM budget, " + kind, worst)
        print(f"{tag}: worst |dA - x.c| / budget = {worst:.4f}")
        assert not viol, f"{tag}: {len(viol)} dot(s) outside the GEMM budget, first (row, centroid) {viol[0]}"
    # (d) |A - C| <= eps for k_km_scan's pair and for the closure / selection pair
    for route, (worst, viol, rows) in gb.check_eps(t["dots"], x, c, t["nx"], t["nc"], t["ncmax"]).items():
        _note(f"|A - C| / eps ({route}), {kind}", worst)
        print(f"{tag}: worst |A - C| / eps ({route}) = {worst:.4f} over {rows} of {n} rows")
        assert not viol, f"{tag}: {len(viol)} pair(s) with |A - C| > eps ({route}), first (row, centroid) {viol[0]}"
        assert rows == n or kind == "mix_1e18"  # (only there do spans pass 1e37)


# ---- near-ties at the scale of eps, end to end ------------------------------------------------------------------------------

NONE = np.uint32(0xFFFFFFFF)
TIES = [pytest.param(gen, dim, k, scale, id=f"{gen}_d{dim}_k{k}_x{scale:g}") for gen in nt.GENERATORS for dim, k, scale in nt.CONFIGS]


def _padded(dim):
    return (dim + 63) // 64 * 64  # the padded dimension of an index


def _conditions(tag, C, eps):
    """Asserted on the CPU restatement before the GPU is asked: at least 40 % of the rows have their two nearest canonical
    distances within 2 eps, and no row has a third centroid within 4 eps.  Returns (near-tie mask, the two nearest)."""
    share, third, near, two = nt.tie_stats(C, eps.astype(np.float64))
    print(f"{tag}: {share:.3f} of {len(C)} rows have their two nearest within 2 eps")
    assert share >= 0.4, (tag, share)
    assert third.size == 0, f"{tag}: rows {third[:10]} have a third centroid within 4 eps"
    return near, two


@pytest.mark.parametrize("gen,dim,k,scale", TIES)
def test_near_ties_nearest_list_of_add(gen, dim, k, scale):
    """IvfRabitqIndex.add's nearest list (KmGemmAssign: k_km_scan and its eps) against kmeans_ref.assign over the rotated rows."""
    import torch
    D = _padded(dim)
    seed = 7100 + dim + k
    cent, x = nt.make(gen, dim, k, scale, gb.eps_km, gb.km_dp(D), seed)
    own = np.arange(k, dtype=np.uint32)  # the index starts with one vector per list: its centroid
    built = rq.builder.train_with_clusters(cent, cent, own, 7, 0, 1, seed + 2, True)
    xd, ad = torch.from_numpy(cent).cuda(), torch.from_numpy(own.astype(np.int32)).cuda()
    idx = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), k, built.t_const, rescale="const")
    try:
        assert idx.padded_dim == D
        crot = idx.debug_copy_index("centroids", np.empty((k, D), f32))
        xrot = np.stack([built.rotate(r) for r in x])
        nx, nc = kmeans_ref.norms(xrot), kmeans_ref.norms(crot)
        span = gb.span_of(nx, nc.max())
        eps = gb.eps_km(gb.km_dp(D), span)
        _conditions(f"add {gen} d{dim}", gb.km_canon_all(xrot, crot, nx, nc), eps)
        want, _ = kmeans_ref.assign(xrot, nx, crot)
        # no row falls back: this path has no counter, so the scan's shortlist is recounted from the front's own output (with
        # one ulp of A and of the threshold to spare) and must fit its 256 entries, with every span below the scan's limit
        t = rk.debug_gemm_shortlist_front(crot, xrot, images=False)
        A, ulp = gb.approx_dist(t["dots"], t["nx"], t["nc"])
        thr = A.min(1) + 2.01 * eps.astype(np.float64) * (1 + 2.0 ** -22)
        cnt = (A <= thr[:, None] + 2 * ulp).sum(1)
        print(f"add {gen} d{dim}: the largest shortlist holds at most {cnt.max()} entries")
        assert cnt.max() <= 256 and (span < gb.SPAN_MAX).all()
        got = idx.add(x, max_chunk_rows=128)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    finally:
        idx.close()
        built.close()


@pytest.mark.parametrize("gen,dim,k,scale", TIES)
def test_near_ties_closure_assignment(gen, dim, k, scale):
    """closure_assign (k_cl_scan, closure_eps) against closure_assign_cpu; the shortlist tap holds what must be in it."""
    Dp = gb.km_dp(dim)
    cent, x = nt.make(gen, dim, k, scale, gb.closure_eps, Dp, 7200 + dim + k)
    nx, nc = gb.km_norm(x), gb.km_norm(cent)
    eps = gb.closure_eps(Dp, gb.span_of(nx, nc.max()))
    near, two = _conditions(f"closure {gen} d{dim}", gb.l2_canon_all(x, cent), eps)
    # k_cl_scan's own decision, restated from the front's output: A in float64, the minimum of each of the 64 lanes' centroids
    t = rk.debug_gemm_shortlist_front(cent, x, images=False)
    A, _ = gb.approx_dist(t["dots"], t["nx"], t["nc"])
    pad = np.full((len(x), -k % 64), np.inf)
    lane_min = np.sort(np.concatenate([A, pad], axis=1).reshape(len(x), -1, 64).min(1), axis=1)
    for M, e in ((1, 0.0), (2, 0.0), (8, 0.15)):
        f0 = mstg.closure_fallbacks()
        lists, counts = rq.closure_assign(x, cent, e, M)
        assert mstg.closure_fallbacks() == f0, f"max_replicas {M}: rows fell back, the shortlist path is not the one under test"
        wl, wc = rq.closure_assign_cpu(x, cent, e, M)
        assert np.array_equal(counts, wc), np.nonzero(counts != wc)[0][:10]
        bad = np.nonzero((lists != wl).any(1))[0]
        assert bad.size == 0, (M, e, bad[:10], lists[bad[0]], wl[bad[0]])
        sl, sl_n = mstg.debug_closure_shortlist(x, cent, M)
        assert (sl_n != NONE).all() and sl_n.max() <= 256
        held = np.zeros(A.shape, bool)
        for i in range(len(x)):
            held[i, sl[i, :sl_n[i]]] = True
        # the shortlist is {c : A(c) <= T + 2.01 eps}, T the M-th smallest lane minimum, with the eps of km_common.hpp: an eps
        # constant that is too small leaves the far member of a near-tie out at max_replicas 1, one that is too large lets
        # others in.  2^-20 of the threshold covers the f32 roundings of A, of 2.01f * eps and of the sum (a few 2^-24 each).
        thr = lane_min[:, M - 1] + 2.01 * eps.astype(np.float64)
        slack = 2.0 ** -20 * thr
        lost = np.nonzero((A <= (thr - slack)[:, None]) & ~held)
        extra = np.nonzero(held & ~(A <= (thr + slack)[:, None]))
        assert lost[0].size == 0, f"max_replicas {M}: shortlists lack (row, centroid) {np.stack(lost, 1)[:5].tolist()} inside T + 2.01 eps"
        assert extra[0].size == 0, f"max_replicas {M}: shortlists hold (row, centroid) {np.stack(extra, 1)[:5].tolist()} beyond T + 2.01 eps"
        # the nearest centroid is always shortlisted; from max_replicas 2 on T is at least the second smallest A, so both
        # members of a near-tie are (completeness: the m first of the exact order)
        r = np.arange(len(x))
        assert held[r, two[:, 0]].all()
        if M >= 2:
            miss = np.nonzero(near & ~held[r, two[:, 1]])[0]
            assert miss.size == 0, f"max_replicas {M}: the shortlists of rows {miss[:10]} lack a member of their near-tie"
        print(f"closure {gen} d{dim} max_replicas {M}: shortlists of {sl_n.min()}..{sl_n.max()} entries, "
              f"{int((near & held[r, two[:, 1]]).sum())} of {int(near.sum())} near-ties held whole")


# An MSTG handle has no rotator and so takes dimensions that are multiples of 16 only: 16 stands in for nt.CONFIGS' 7.
MSTG_TIES = [pytest.param(gen, max(dim, 16), k, scale, id=f"{gen}_d{max(dim, 16)}_k{k}_x{scale:g}")
             for gen in nt.GENERATORS for dim, k, scale in nt.CONFIGS]


@pytest.mark.parametrize("gen,dim,k,scale", MSTG_TIES)
def test_near_ties_mstg_list_selection(gen, dim, k, scale):
    """mstg_search's list selection (k_ms_scan, closure_eps at the index's padded dimension) against select_lists_cpu."""
    seed = 7300 + dim + k
    Dp = gb.km_dp(dim)  # (no rotator: the index's padded dimension is dim)
    cent, x = nt.make(gen, dim, k, scale, gb.closure_eps, Dp, seed)
    nx, nc = gb.km_norm(x), gb.km_norm(cent)
    eps = gb.closure_eps(Dp, gb.span_of(nx, nc.max()))
    _conditions(f"mstg {gen} d{dim}", gb.l2_canon_all(x, cent), eps)
    built = mc.given_centroids_case(3, np.concatenate([cent, x]), cent, seed + 1)  # (what the lists hold does not matter here)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        assert idx.padded_dim == dim
        for ef, pe in ((1, 1e9), (2, 0.0), (150, 0.6)):
            f0 = mstg.search_fallbacks()
            _, _, _, li, lc = rq.mstg_search(idx, x, 10, ef, pe, return_lists=True)
            assert mstg.search_fallbacks() == f0, f"ef {ef}: queries fell back, the shortlist path is not the one under test"
            rl, rc = rq.select_lists_cpu(x, cent, ef, pe)
            assert np.array_equal(lc, rc), (ef, pe, np.nonzero(lc != rc)[0][:10])
            bad = np.nonzero((li != rl).any(1))[0]
            assert bad.size == 0, (ef, pe, bad[:10], li[bad[0]], rl[bad[0]])
    finally:
        idx.close()
        built.close()
