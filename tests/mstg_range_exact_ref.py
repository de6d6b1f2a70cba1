"""The exact MSTG range search (options "mstg_range_exact" / "mstg_range_exact_bits" on rbq_mstg_range_batch; include/ext/rbq_mstg_range.h,
DESIGN.md section 38) restated.  No GPU.  The candidates are mstg_range_ref.range_rows at the candidate radius r with distinct ids
and unlimited capacity; every kept id is scored by mstg_rerank_ref.distances (the oracle's canonical sums, negated for inner
product; NaN without a raw row); an id matches iff that distance is finite and < x; the matches keep the scan order."""
import numpy as np

import mstg_range_ref as rref
import mstg_rerank_ref as kref


def stored_rows(x, raw):
    """(the rows as they are attached, the rows as the scorer sees them: f32) for raw = "f32" | "f16" | "bf16\""""
    x = np.ascontiguousarray(x, np.float32)
    if raw == "bf16":
        return kref.round_bf16(x), kref.widen_bf16(kref.round_bf16(x))
    return (x, x) if raw == "f32" else (x.astype(np.float16), x.astype(np.float16).astype(np.float32))


def candidate_distances(cands, wide_q, wide_raw, metric, r):
    """per query (the distinct candidates at r in scan order, their exact distances), or None where the query is over the limit"""
    ci, _, cc, _ = rref.range_rows(cands, r, 1, max(max(len(c[0]) for c in cands), 1))
    return [None if cc[i] == rref.U32_MAX else (ci[i, :cc[i]], kref.distances(wide_q[i], wide_raw, ci[i, :cc[i]], metric)) for i in range(len(cands))]


def exact_rows(cands, wide_q, wide_raw, metric, r, x, cap):
    """(ids [nq][cap] u64, exact score bits [nq][cap] u32, counts [nq] u32, distinct candidates per query [nq] i64)"""
    nq = len(cands)
    ids, bits = np.full((nq, cap), rref.NONE64, np.uint64), np.full((nq, cap), rref.NAN_BITS, np.uint32)
    cnt, ncand = np.zeros(nq, np.uint32), np.zeros(nq, np.int64)
    for i, kd in enumerate(candidate_distances(cands, wide_q, wide_raw, metric, r)):
        if kd is None:                                           # over the limit: nothing is scored on a prefix
            cnt[i], ncand[i] = rref.U32_MAX, -1
            continue
        with np.errstate(invalid="ignore"):
            m = np.isfinite(kd[1]) & (kd[1] < np.float32(x))     # (never true against a NaN x)
        k = min(int(m.sum()), cap)
        ids[i, :k], bits[i, :k], cnt[i], ncand[i] = kd[0][m][:k], kd[1][m][:k].view(np.uint32), m.sum(), len(m)
    return ids, bits, cnt, ncand


def kth_exact_radius(cands, wide_q, wide_raw, metric, r, k=20):
    """the median over the queries of the k-th smallest exact distance among the candidates at r (queries with fewer left out)"""
    kth = [np.sort(kd[1])[k - 1] for kd in candidate_distances(cands, wide_q, wide_raw, metric, r) if kd is not None and len(kd[1]) >= k]
    return np.float32(np.median(np.asarray(kth, np.float32)))
