"""The error budget of the approximate ranking GEMM (rank_mfma.hpp header) restated in numpy, shared by
test_gpu_rank_bound.py (which holds the GPU's score rows to it) and test_rank_bound_host.py (which shows that it
rejects the rows a broken GEMM would write).

  bf16_split      the kernels' split of an f32 into two bf16 halves (types.hpp bf16_rne / bf16_split)
  canonical       the reference's l2_distance_sqr / dot in their lane order (oracle ref_l2_distance_sqr / ref_dot)
  exact_scores    the float64 value s64 of every (query, list) score the GEMM approximates
  gemm_budget     the GEMM's own share of eps: (4 D + 16) u + 3.02 * 2^-16, times |q|^2 + |c|^2
  select_eps      eps exactly as k_select_mfma computes it in f32
  check_rows      |A - s64| <= gemm_budget for every pair; the worst ratio and the violating pairs
  rewritten       the IP entries the selection overwrote with their canonical L2 distance (left out of the check)
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of f32
SPLIT_REL = 2.0 ** -16  # |x - hi - lo| <= 2^-16 |x| for the bf16 split of a normal x
SPLIT_ABS = 2.0 ** -134  # ... plus half the spacing of bf16 subnormals, the floor of lo's rounding


def bf16_rne(x):
    """f32 -> bf16 bits, round to nearest even; NaN keeps its sign and is made quiet, inf stays inf."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_split(x):
    """(hi, lo) bits with x = hi + lo + r: hi = bf16(x), lo = bf16(x - hi), the subtraction in f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = bf16_rne(x - bf16_to_f32(hi))
    return hi, lo


def split_residual_ok(x, hi, lo):
    """Mask of the finite elements of x whose split leaves |x - hi - lo| <= 2^-16 |x| + 2^-134 (non-finite: True)."""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(x.astype(np.float64) - bf16_to_f32(hi).astype(np.float64) - bf16_to_f32(lo).astype(np.float64))
    return ~fin | (r <= SPLIT_REL * np.abs(x.astype(np.float64)) + SPLIT_ABS)


def canonical(q, c, metric):
    """The reference's f32 score of each row pair (q[i], c[i]) in its own order: 8 strided lanes of unfused
    multiply-then-add, the lanes summed 0..7 starting from -0.0, then the scalar tail (oracle/rbq_ref.c)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    P, D = q.shape
    main = D // 8 * 8
    acc = np.zeros((P, 8), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(0, main, 8):
            a, b = q[:, i:i + 8], c[:, i:i + 8]
            if metric == 0:
                d = a - b
                acc = acc + d * d
            else:
                acc = acc + a * b
        s = np.full(P, -0.0 if main else 0.0, np.float32)
        for lane in range(8 if main else 0):
            s = s + acc[:, lane]
        for i in range(main, D):
            p = (q[:, i] - c[:, i]) ** 2 if metric == 0 else q[:, i] * c[:, i]
            s = s + p.astype(np.float32)
    return s


def exact_scores(rot, cent, metric):
    """(s64, |q|^2 + |c|^2) in float64 for every (query, list) pair: |q|^2 + |c|^2 - 2 q.c (L2) or q.c (IP)."""
    q = np.asarray(rot, dtype=np.float64)
    c = np.asarray(cent, dtype=np.float64)
    qn, cn = np.einsum("ij,ij->i", q, q), np.einsum("ij,ij->i", c, c)
    dot = q @ c.T
    norms = qn[:, None] + cn[None, :]
    return (norms - 2.0 * dot if metric == 0 else dot), norms


def gemm_budget(D, norms):
    """The GEMM's share of the header's bound: accumulation of 3 D exact products and the norm terms in f32 (even with
    a truncating adder), plus the terms the bf16 split drops."""
    return ((4.0 * D + 16.0) * U + 3.02 * SPLIT_REL) * norms


def select_eps(D, qnorm2, cnorm2_max):
    """k_select_mfma's eps (rank_mfma.hpp), evaluated in f32 like the kernel."""
    f = np.float32
    base = (f(6.0) * f(D) + f(16.0)) * f(5.9604645e-8) + f(4.0) * f(1.52587890625e-5)
    return (base * (np.asarray(qnorm2, np.float32) + f(cnorm2_max))) * f(1.001)


def cnorm2_max_of(cnorm2):
    """The index's cnorm2_max: the largest finite |c|^2, rounded up as the library does."""
    c = np.asarray(cnorm2, np.float32)
    c = c[np.isfinite(c)]
    return np.float32((float(c.max()) if c.size else 0.0) * 1.000001)


def rewritten(A, rot, cent, qi, ci, l2=None):
    """Mask of the IP pairs (qi, ci) whose entry the selection rewrote: for IP it overwrites the lists it rescored with
    their canonical L2 distance, so an entry is taken for rewritten only if it equals that distance bit for bit.  Only
    entries near the float64 distance `l2` of their pair (computed when not given) are evaluated in canonical order."""
    A = np.asarray(A, np.float32)
    D = np.shape(rot)[1]
    if l2 is None:
        l2 = ((np.asarray(rot, np.float64)[qi] - np.asarray(cent, np.float64)[ci]) ** 2).sum(1)
    a = A[qi, ci].astype(np.float64)
    with np.errstate(invalid="ignore"):
        near = np.abs(a - l2) <= 2.0 * (D + 8) * U * l2 + 1e-30  # canonical l2 is within gamma_(D+8) of the exact one
    out = np.zeros(qi.shape, bool)
    k = np.nonzero(near)[0]
    for i in range(0, k.size, 65536):
        j = k[i:i + 65536]
        out[j] = A[qi[j], ci[j]].view(np.uint32) == canonical(np.asarray(rot)[qi[j]], np.asarray(cent)[ci[j]], 0).view(np.uint32)
    return out


def check_rows(A, rot, cent, metric, D, skip_rewritten=False):
    """Hold a score matrix A [nq][nlist] to |A - s64| <= gemm_budget.  skip_rewritten (IP only): leave out the entries
    the selection rewrote (rewritten()).  Returns (worst ratio of the checked pairs, violating pairs, pairs left out)."""
    A = np.asarray(A, np.float32)
    worst, viol, skipped = 0.0, [], 0
    for r0 in range(0, A.shape[0], 256):  # (row blocks: the float64 temporaries of 4096 x 17000 rows would not be small)
        s64, norms = exact_scores(rot[r0:r0 + 256], cent, metric)
        budget = gemm_budget(D, norms)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(A[r0:r0 + 256].astype(np.float64) - s64)
        checked = np.ones(err.shape, bool)
        if skip_rewritten and metric == 1:
            qi, ci = np.nonzero(checked)
            checked[qi, ci] = ~rewritten(A, rot, cent, qi + r0, ci, (norms - 2.0 * s64)[qi, ci])
            skipped += int((~checked).sum())
        bad = checked & ~(err <= budget)  # NaN and inf are violations
        qi, ci = np.nonzero(bad)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(checked, err / np.maximum(budget, np.finfo(np.float64).tiny), 0.0)
        if ratio.size:
            worst = max(worst, float(np.max(np.where(np.isnan(ratio), np.inf, ratio))))
        viol += list(zip((qi + r0).tolist(), ci.tolist()))
    return worst, viol, skipped
