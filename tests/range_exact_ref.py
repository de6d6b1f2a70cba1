"""The exact range search (options "range_exact" / "range_exact_radius_bits") restated: the candidates are
the matches of the range search's restatement (range_ref.range_query at the estimate's radius r, in its scan order, with its
counters), each is scored by the pooled rerank's restatement (rerank_pool_ref.exact_scores: the oracle's canonical
l2_distance_sqr / dot against the raw row, NaN 0x7fc00000 without one), and a candidate matches iff exact distance < x (L2) or
exact dot product > x (inner product).  16-bit rows and queries enter widened (rerank_f16_ref.widen).  Nothing here is taken from
the library under test."""
import numpy as np

import range_ref
import rerank_f16_ref
from rerank_pool_ref import exact_scores

F32 = np.float32
rows = range_ref.rows        # (ids [nq, cap], score bits [nq, cap], totals) of a batch's reference results at capacity cap
diag_of = range_ref.diag_of  # the candidate scan's counters: they depend on neither x nor the capacity


def widened(a, dtype=None):
    """f32 values of rows or queries as the library reads them: f32 as they are, "f16" / "bf16" bit patterns (or a float16 array)
    widened exactly"""
    if dtype in (None, "f32"):
        return np.ascontiguousarray(a, F32)
    a = np.ascontiguousarray(a)
    return rerank_f16_ref.widen(a.view(np.uint16), dtype)


def unbounded_radius(metric):
    """the candidate radius that admits every finite distance"""
    return F32(np.inf) if metric == 0 else F32(-np.inf)


def passes(scores, x, metric):
    """rule 3: exact distance < x (L2), exact dot product > x (inner product); NaN never"""
    with np.errstate(invalid="ignore"):
        return scores < F32(x) if metric == 0 else scores > F32(x)


def from_candidates(cand, q, raw, x, metric):
    """one query: cand = range_ref.range_query's (ids, estimated scores, counters) -> (ids, exact scores, counters)"""
    ids, _, counters = cand
    ex = exact_scores(q, raw, ids, metric)
    keep = passes(ex, x, metric)
    return ids[keep], ex[keep].astype(F32), counters


def range_exact_query(built, q, raw, x, r, nprobe, allowed=None):
    """One query (f32, widened) against raw rows (f32, widened; raw.shape[0] = n_raw) -> (ids u64, exact scores f32, counters), in
    scan order."""
    metric = int(built.header.metric)
    return from_candidates(range_ref.range_query(built, q, r, nprobe, allowed), q, raw, x, metric)


def range_exact_batch(built, queries, raw, x, r, nprobe, allowed=None):
    raw = np.ascontiguousarray(raw, F32)
    return [range_exact_query(built, q, raw, x, r, nprobe, allowed) for q in np.ascontiguousarray(queries, dtype=F32)]


def kth_exact_score(built, q, raw, k, nprobe):
    """x: query q's k-th best (1-based) exact score over the vectors of its probed lists — with distinct scores, the k - 1 better
    ones pass it"""
    metric = int(built.header.metric)
    ids = np.concatenate([i for i, _, _ in range_ref.probed_vectors(built, q, nprobe)])
    ex = exact_scores(q, np.ascontiguousarray(raw, F32), ids, metric)
    ex = ex[~np.isnan(ex)]
    s = np.sort(ex if metric == 0 else -ex)[k - 1]
    return F32(s if metric == 0 else -s)
