"""CPU side of the GEMM-shortlist front end's bounds (tests/gemm_shortlist_bound.py): the numpy restatements are pinned to
hand-evaluated f32 values and to the project's other restatements, and the checkers that test_gpu_gemm_shortlist_bound.py
applies to the tap rbq_debug_gemm_shortlist_front reject what a broken front end would write."""
import numpy as np
import pytest

import gemm_shortlist_bound as gb
import kmeans_ref
import rank_bound as rb
from conftest import make_dataset

f32 = np.float32
SCALES = [1.0, 1e-4, 1e4]


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


# ---- the restatements ---------------------------------------------------------------------------------------------------

def test_km_dp():
    assert [gb.km_dp(d) for d in (1, 31, 32, 33, 64, 65, 2500)] == [32, 32, 32, 64, 64, 96, 2528]


@pytest.mark.parametrize("Dp,span,km,cl", [
    # Dp 32: 32 * 2^-21 + 2^-14 = 5 * 2^-16, times 1025 / 1024; (384 * 2^-24 + 2^-14) = 11 * 2^-17, times 65 / 64; 2^-100 rounds away
    (32, 1.0, 5125.0 * 2.0 ** -26, 715.0 * 2.0 ** -23),
    # Dp 2528 (dim 2500), span 3 * 2^20: 83 * 2^-16 * 3 * 2^20 = 3984, times 1025 / 1024; 26368 * 2^-24 * 3 * 2^20 = 4944, times 65 / 64
    (2528, 3.0 * 2.0 ** 20, 3987.890625, 5021.25),
    # span 0 (rows and centroids all zero): the floor 2^-100 alone
    (96, 0.0, 2.0 ** -100, 2.0 ** -100),
])
def test_eps_restatements_equal_hand_evaluated_f32(Dp, span, km, cl):
    for fn, want in ((gb.eps_km, km), (gb.closure_eps, cl)):
        got = fn(Dp, f32(span))
        assert got.dtype == f32 and _bits(got) == _bits(f32(want)), (fn.__name__, Dp, span, float(got), want)
        assert float(f32(want)) == want  # (the hand value is an f32)
    # an array of spans gives the scalar's values; span at the scans' limit still gives a finite eps
    v = gb.closure_eps(Dp, np.array([span, span], f32))
    assert v.shape == (2,) and (_bits(v) == _bits(f32(cl))).all()
    assert np.isfinite(gb.closure_eps(16384, f32(9.99e36))) and np.isfinite(gb.eps_km(16384, f32(9.99e36)))


def test_split_images_are_zero_padded():
    x = np.array([[1.0, 1.0 + 2.0 ** -8, -3.0]], f32)
    hi, lo = gb.split_images(x)
    assert hi.shape == lo.shape == (1, 32)
    assert hi[0, :3].tolist() == [0x3F80, 0x3F80, 0xC040] and lo[0, :3].tolist() == [0, 0x3B80, 0]
    assert not hi[0, 3:].any() and not lo[0, 3:].any()


def test_canonical_forms_equal_the_other_restatements():
    """km_norm / km_canon_all against tests/kmeans_ref.py, l2_canon_all against rank_bound.canonical, bit for bit."""
    rng = np.random.default_rng(11)
    for dim in (1, 7, 8, 13, 100):
        x = rng.standard_normal((9, dim)).astype(f32)
        c = rng.standard_normal((21, dim)).astype(f32)
        nx, nc = gb.km_norm(x), gb.km_norm(c)
        assert np.array_equal(_bits(nx), _bits(kmeans_ref.norms(x)))
        C = gb.km_canon_all(x, c, nx, nc)
        best, bestd = kmeans_ref.assign(x, nx, c)
        assert np.array_equal(_bits(C[np.arange(9), best]), _bits(bestd)) and np.array_equal(C.min(1), bestd)
        L = gb.l2_canon_all(x, c)
        want = rb.canonical(np.repeat(x, 21, axis=0), np.tile(c, (9, 1)), 0).reshape(9, 21)
        assert np.array_equal(_bits(L), _bits(want)), dim


def test_approx_dist_allows_one_ulp_of_the_fma():
    """A in float64 is within one f32 ulp of the f32 fmaf, clamped at 0, and never NaN."""
    nx, nc = np.array([3.0, 1e-3], f32), np.array([5.0, 0.25, 7.0], f32)
    d = np.array([[3.9999, 0.1, 6.0], [1.0, 1e-5, 1e-7]], f32)
    A, ulp = gb.approx_dist(d, nx, nc)
    s = (nx[:, None] + nc[None, :]).astype(np.float64)
    assert np.array_equal(A, np.maximum(s - 2.0 * d.astype(np.float64), 0.0))
    assert (A >= 0).all() and A[0, 2] == 0.0  # (3 + 7 - 12 < 0: clamped)
    assert (np.abs(A.astype(f32).astype(np.float64) - A) <= ulp).all() and ulp[0, 2] == 2.0 ** -149


# ---- the checkers have teeth ----------------------------------------------------------------------------------------------

def _operands(dim, scale, n=130, k=260):
    x = (make_dataset(n, dim, 16, 900 + dim) * f32(scale)).astype(f32)
    c = (make_dataset(k, dim, 16, 901 + dim) * f32(scale)).astype(f32)
    return x, c


def _planes(x, pad_from_next_row=False):
    """The hi / lo planes of x as float64 [rows][Dp].  pad_from_next_row: the padding columns hold what follows the row in
    memory (the image of a split that walked the rows with stride dim but wrote Dp columns)."""
    x = np.ascontiguousarray(x, f32)
    n, dim = x.shape
    Dp = gb.km_dp(dim)
    if pad_from_next_row:
        flat = np.concatenate([x.reshape(-1), np.zeros(Dp, f32)])
        x = np.stack([flat[r * dim:r * dim + Dp] for r in range(n)])
    hi, lo = gb.split_images(x)
    return rb.bf16_to_f32(hi).astype(np.float64), rb.bf16_to_f32(lo).astype(np.float64)


def _split_dots(x, c, drop=None, pad_from_next_row=False):
    """What the split-bf16 GEMM computes from the images, qh.ch + qh.cl + ql.ch exactly and rounded once, or a broken one."""
    qh, ql = _planes(x, pad_from_next_row)
    ch, cl = _planes(c, pad_from_next_row)
    if drop == "last_slab":
        qh, ql, ch, cl = (a[:, :-32] for a in (qh, ql, ch, cl))
    d = qh @ ch.T
    if drop != "qh_cl":
        d = d + qh @ cl.T
    if drop != "ql_ch":
        d = d + ql @ ch.T
    return d.astype(f32)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dim", [33, 100])
def test_checkers_accept_the_split_gemm(dim, scale):
    x, c = _operands(dim, scale)
    nx, nc = gb.km_norm(x), gb.km_norm(c)
    d = _split_dots(x, c)
    worst, viol = gb.check_dots(d, x, c)
    assert not viol and worst < 0.5, (worst, viol[:5])
    for route, (w, bad, rows) in gb.check_eps(d, x, c, nx, nc, nc.max()).items():
        assert not bad and w < 0.5 and rows == x.shape[0], (route, w, bad[:5])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dim", [33, 100])
@pytest.mark.parametrize("fault", ["ql_ch", "qh_cl", "last_slab", "padding"])
def test_gemm_budget_rejects_a_broken_front(fault, dim, scale):
    x, c = _operands(dim, scale)
    d = _split_dots(x, c, pad_from_next_row=True) if fault == "padding" else _split_dots(x, c, drop=fault)
    worst, viol = gb.check_dots(d, x, c)
    assert viol and worst > 1.0, f"{fault}: accepted (worst ratio {worst})"


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dim", [33, 100])
def test_eps_check_rejects_a_norm_from_another_row(dim, scale):
    """nx of row r + 128 (a later pass's row) in place of row r's: |A - C| <= eps fails on both routes."""
    x, c = _operands(dim, scale)
    nx, nc = gb.km_norm(x), gb.km_norm(c)
    d = _split_dots(x, c)
    canon = {"km": gb.km_canon_all(x, c, nx, nc), "closure": gb.l2_canon_all(x, c)}
    wrong = np.roll(nx, -128)
    for route, (w, bad, _) in gb.check_eps(d, x, c, wrong, nc, nc.max(), canon=canon).items():
        assert bad and w > 1.0, f"{route}: accepted (worst ratio {w})"
        assert {0, 1} <= {r for r, _ in bad}  # rows 0 and 1 took the norms of rows 128 and 129


def test_eps_check_leaves_out_rows_the_scans_send_to_the_fallback():
    x = np.array([[4e18, 0.0], [1.0, 1.0]], f32)
    c = np.array([[1.0, 2.0]], f32)
    nx, nc = gb.km_norm(x), gb.km_norm(c)
    assert nx[0] >= gb.SPAN_MAX
    d = (x.astype(np.float64) @ c.astype(np.float64).T).astype(f32)
    for route, (w, bad, rows) in gb.check_eps(d, x, c, nx, nc, nc.max()).items():
        assert rows == 1 and not bad and w < 1.0, (route, w, bad)
