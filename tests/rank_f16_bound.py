"""The one-product f16 ranking GEMM (rank_mfma.hpp header, "ONE f16 PRODUCT") restated in numpy, shared by
test_gpu_rank_f16.py (which holds the GPU's images, residuals and score rows to it) and test_rank_f16_host.py (which shows
against float64 that the budget holds for any summation order and rejects the rows a broken GEMM would write).

  f16_image     np.float16 (round to nearest even), then every half below the smallest normal stored as a signed zero
  f16_value     the f32 value of image bits
  resid64       |x - f16(x)| per row in float64, from the bits stored
  resid32       the same as the kernels round it up to f32
  rc_max_of, cnorm_max_of, gate   what the host keeps of a centroid image, and whether the index qualifies
  select_eps    eps as k_select_mfma computes it in f32 on this route
  gemm_budget   (4 D + 16) u (|q|^2 + |c|^2) + 2 (|ql||c| + |qh||cl|)
  check_rows    |A - s64| <= gemm_budget for every pair; the worst ratio and the violating pairs
"""
import numpy as np

import rank_bound as rb

U = rb.U
GATE = 2.0 ** -11  # rc_max <= GATE * sqrt(cnorm2_max)


def f16_image(x, flush=True):
    """f16 bits of x.  flush=False leaves IEEE subnormal halves in place (NOT what is stored: host tests only)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        bits = x.astype(np.float16).view(np.uint16).copy()
    if flush:
        sub = (bits & 0x7C00) == 0
        bits[sub] &= 0x8000
    return bits


def f16_value(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32)


def resid64(x, bits):
    """|x - f16(x)| per row in float64 (inf or NaN where the image is not finite)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.asarray(x, np.float32).astype(np.float64) - f16_value(bits).astype(np.float64)
        return np.sqrt((r * r).sum(-1))


def resid32(x, bits):
    """The residual as the kernels store it: the float64 value times 1.000001, rounded to f32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (resid64(x, bits) * 1.000001).astype(np.float32)


def residual_ok(got, want64):
    """A stored residual is at or above the float64 value and within 1e-5 relative of it (both not finite: fine)."""
    got = np.asarray(got, np.float32).astype(np.float64)
    fin = np.isfinite(want64)
    with np.errstate(invalid="ignore"):
        return np.where(fin, (got >= want64) & (got <= want64 * (1.0 + 1e-5)), ~np.isfinite(got))


def rc_max_of(resid):
    """The largest stored centroid residual (they are rounded up already; not finite ones fail the gate instead)."""
    r = np.asarray(resid, np.float32)
    r = r[np.isfinite(r)]
    return np.float32(r.max() if r.size else 0.0)


def cnorm_max_of(cnorm2):
    """sqrt(cnorm2_max) rounded up, as the host computes it from the largest finite |c|^2."""
    c = np.asarray(cnorm2, np.float32)
    c = c[np.isfinite(c)]
    mx = float(c.max()) if c.size else 0.0
    return np.float32(np.sqrt(mx * 1.000001) * 1.000001)


def gate(resid, cnorm2):
    """The index qualifies: every stored half (hence every residual) and every norm finite, and rc_max <= 2^-11 sqrt(cnorm2_max)."""
    r, c = np.asarray(resid, np.float32), np.asarray(cnorm2, np.float32)
    if not (np.isfinite(r).all() and np.isfinite(c).all()):
        return False
    return float(rc_max_of(r)) <= GATE * float(cnorm_max_of(c))


def select_eps(D, qnorm2, cnorm2_max, rq, cnorm_max, rc_max):
    """k_select_mfma's eps on the one-product route, evaluated in f32 like the kernel."""
    f = np.float32
    qnorm2, rq = np.asarray(qnorm2, f), np.asarray(rq, f)
    with np.errstate(invalid="ignore", over="ignore"):
        base = ((f(6.0) * f(D) + f(16.0)) * f(5.9604645e-8)) * (qnorm2 + f(cnorm2_max))
        qn = np.sqrt(qnorm2) * f(1.0000002)
        return (base + f(2.01) * (rq * f(cnorm_max) + (qn + rq) * f(rc_max))) * f(1.001)


def gemm_budget(D, rot, cent, qbits=None, cbits=None):
    """[nq][nlist] budget of the score: accumulation of D exact products and the norm terms in f32 (even with a truncating
    adder), plus twice the Cauchy-Schwarz bound of the dropped terms ql.c + qh.cl.  The images default to f16_image."""
    qbits = f16_image(rot) if qbits is None else qbits
    cbits = f16_image(cent) if cbits is None else cbits
    q, c = np.asarray(rot, np.float64), np.asarray(cent, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        qn, cn = np.sqrt((q * q).sum(1)), np.sqrt((c * c).sum(1))
        qh = np.sqrt((f16_value(qbits).astype(np.float64) ** 2).sum(1))
        ql, cl = resid64(rot, qbits), resid64(cent, cbits)
        norms = (qn * qn)[:, None] + (cn * cn)[None, :]
        return (4.0 * D + 16.0) * U * norms + 2.0 * (ql[:, None] * cn[None, :] + qh[:, None] * cl[None, :])


def check_rows(A, rot, cent, metric, D, skip_rewritten=False, qbits=None, cbits=None):
    """Hold a score matrix A [nq][nlist] to |A - s64| <= gemm_budget, as rank_bound.check_rows does for split-bf16.
    Returns (worst ratio of the checked pairs, violating pairs, pairs left out)."""
    A = np.asarray(A, np.float32)
    qbits = f16_image(rot) if qbits is None else qbits
    cbits = f16_image(cent) if cbits is None else cbits
    worst, viol, skipped = 0.0, [], 0
    for r0 in range(0, A.shape[0], 256):
        s64, norms = rb.exact_scores(rot[r0:r0 + 256], cent, metric)
        budget = gemm_budget(D, rot[r0:r0 + 256], cent, qbits[r0:r0 + 256], cbits)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(A[r0:r0 + 256].astype(np.float64) - s64)
        checked = np.ones(err.shape, bool)
        if skip_rewritten and metric == 1:
            qi, ci = np.nonzero(checked)
            checked[qi, ci] = ~rb.rewritten(A, rot, cent, qi + r0, ci, (norms - 2.0 * s64)[qi, ci])
            skipped += int((~checked).sum())
        bad = checked & ~(err <= budget)  # NaN and inf are violations
        qi, ci = np.nonzero(bad)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(checked, err / np.maximum(budget, np.finfo(np.float64).tiny), 0.0)
        if ratio.size:
            worst = max(worst, float(np.max(np.where(np.isnan(ratio), np.inf, ratio))))
        viol += list(zip((qi + r0).tolist(), ci.tolist()))
    return worst, viol, skipped
