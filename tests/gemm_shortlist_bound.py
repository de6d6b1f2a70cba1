"""The GEMM-shortlist front end (k_gemm_shortlist.hip) and the error bounds its three scan kernels rely on, restated in
numpy.  Shared by test_gpu_gemm_shortlist_bound.py (which holds the tap rbq_debug_gemm_shortlist_front to them) and
test_gemm_shortlist_bound_host.py (which shows that they reject what a broken front end would write).  Every number is the
kernels' own text (km_common.hpp, k_gemm_shortlist.hip) or comes from rank_bound.py.

  km_dp            the padded dimension of the split images: dim rounded up to 32 (launch.hpp)
  split_images     bf16_split of every row, zeros beyond dim (k_km_split)
  km_norm          the sequential unfused f32 norm (km_common.hpp)
  approx_dist      A = max(fma(-2, d, nx + nc), 0) in float64, and the one f32 ulp its single rounding may move it
  eps_km           k_km_scan's eps, f32 operation by f32 operation
  closure_eps      the eps of k_cl_scan and k_ms_scan (km_common.hpp), likewise
  km_canon_all     canonical form 1: (nx + nc) - 2 * (sequential dot), clamped at 0 (k_gemm_shortlist.hip km_canon)
  l2_canon_all     canonical form 2: math::l2_distance_sqr's 8-lane diff-squared order (closure_ref.l2_rows)
  check_dots       the GEMM's own float64 budget for the raw dots: rank_bound.check_rows, inner-product form, D = Dp
  check_eps        |A - C| <= eps for both (canonical form, eps) pairs; the worst ratio and the violating pairs of each
"""
import numpy as np

import closure_ref
import rank_bound as rb

f32 = np.float32
SPAN_MAX = f32(1e37)  # the scans send a row with !(span < 1e37f) to the fallback
ROUTES = ("km", "closure")


def km_dp(dim):
    return (int(dim) + 31) // 32 * 32


def split_images(x):
    """(hi, lo) u16 [rows][Dp]: bf16_split of the coordinates, zero beyond dim."""
    x = np.ascontiguousarray(x, dtype=f32)
    n, dim = x.shape
    hi = np.zeros((n, km_dp(dim)), np.uint16)
    lo = np.zeros((n, km_dp(dim)), np.uint16)
    hi[:, :dim], lo[:, :dim] = rb.bf16_split(x)
    return hi, lo


def km_norm(x):
    """km_norm of every row: s = s + x[j] * x[j] in coordinate order, product and sum each rounded to f32."""
    x = np.ascontiguousarray(x, dtype=f32)
    s = np.zeros(x.shape[0], f32)
    with np.errstate(over="ignore", under="ignore"):
        for j in range(x.shape[1]):
            s = s + x[:, j] * x[:, j]
    return s


def approx_dist(dots, nx, nc):
    """(A, ulp): km_approx_dist for every pair.  nx + nc is the kernel's f32 sum; the fmaf is evaluated in float64, where
    -2 d + s carries 2^-53 of relative error instead of the fmaf's single rounding to f32, so the kernel's A lies within one
    f32 ulp of this A (ulp: the spacing of f32 at A, 2^-149 for a subnormal): the checks allow that much on top of eps."""
    with np.errstate(over="ignore"):
        s = (np.asarray(nx, f32)[:, None] + np.asarray(nc, f32)[None, :]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        A = np.maximum(s - 2.0 * np.asarray(dots, f32).astype(np.float64), 0.0)
        a32 = np.minimum(A, float(np.finfo(f32).max)).astype(f32)
        ulp = np.abs(np.spacing(a32)).astype(np.float64)
    return A, ulp


def span_of(nx, ncmax):
    with np.errstate(over="ignore"):
        return np.asarray(nx, f32) + f32(ncmax)


def eps_km(Dp, span):
    """k_km_scan: ((float)Dp * 2^-21 + 2^-14) * span * (1 + 2^-10) + 2^-100, every operation rounded to f32."""
    span = np.asarray(span, f32)
    with np.errstate(over="ignore"):
        return (f32(Dp) * f32(4.76837158203125e-07) + f32(6.103515625e-05)) * span * f32(1.0009765625) + f32(7.888609052210118e-31)


def closure_eps(Dp, span):
    """km_common.hpp: ((float)(10 Dp + 64) * 2^-24 + 2^-14) * span * (1 + 2^-6) + 2^-100, every operation rounded to f32."""
    span = np.asarray(span, f32)
    with np.errstate(over="ignore"):
        return (f32(10 * int(Dp) + 64) * f32(5.9604644775390625e-08) + f32(6.103515625e-05)) * span * f32(1.015625) \
            + f32(7.888609052210118e-31)


EPS = {"km": eps_km, "closure": closure_eps}


def km_canon_all(x, c, nx, nc):
    """km_canon of every (row, centroid) pair [n][k]: the dot as a sequential unfused f32 chain in coordinate order."""
    x = np.ascontiguousarray(x, dtype=f32)
    c = np.ascontiguousarray(c, dtype=f32)
    dot = np.zeros((x.shape[0], c.shape[0]), f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(x.shape[1]):
            dot = dot + x[:, j:j + 1] * c[None, :, j]
        d = (np.asarray(nx, f32)[:, None] + np.asarray(nc, f32)[None, :]) - f32(2.0) * dot
    return np.where(d < 0, f32(0.0), d)


def l2_canon_all(x, c):
    """math::l2_distance_sqr of every (row, centroid) pair [n][k] in its 8-lane order (closure_ref.l2_rows, row by row)."""
    x = np.ascontiguousarray(x, dtype=f32)
    c = np.ascontiguousarray(c, dtype=f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.stack([closure_ref.l2_rows(x[i], c) for i in range(x.shape[0])]) if x.shape[0] else np.empty((0, c.shape[0]), f32)


def check_dots(dots, x, c):
    """rank_bound.check_rows on the raw dots: |dA - x.c| <= ((4 Dp + 16) u + 3.02 * 2^-16)(|x|^2 + |c|^2)."""
    worst, viol, _ = rb.check_rows(dots, np.asarray(x, f32), np.asarray(c, f32), 1, km_dp(np.shape(x)[1]))
    return worst, viol


def check_eps(dots, x, c, nx, nc, ncmax, canon=None):
    """Hold every pair of every row the scans would scan (span < 1e37) to |A - C| <= eps + ulp(A) for both routes.
    Returns {route: (worst (|A - C| - ulp) / eps, violating pairs, rows checked)}.  `canon`: {route: C [n][k]} when the
    caller has them already."""
    Dp = km_dp(np.shape(x)[1])
    A, ulp = approx_dist(dots, nx, nc)
    span = span_of(nx, ncmax)
    rows = span < SPAN_MAX
    out = {}
    for route in ROUTES:
        if canon is not None and route in canon:
            C = canon[route]
        else:
            C = km_canon_all(x, c, nx, nc) if route == "km" else l2_canon_all(x, c)
        eps = EPS[route](Dp, span).astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.maximum(np.abs(A - C.astype(np.float64)) - ulp, 0.0)
            bad = rows[:, None] & ~(err <= eps)  # (NaN and inf are violations)
            ratio = np.where(rows[:, None], err / eps, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        qi, ci = np.nonzero(bad)
        out[route] = (float(ratio.max()) if ratio.size else 0.0, list(zip(qi.tolist(), ci.tolist())), int(rows.sum()))
    return out
