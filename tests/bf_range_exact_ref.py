"""The exact brute-force range search (rbq_bf_range_exact_batch) restated per query: the candidates are
bf_range_ref.row's matches at the candidate radius r; each is scored by rerank_pool_ref.exact_scores (the oracle's canonical
sums) against the rows as the scorer sees them (rerank_f16_ref.widen of what is stored); a candidate matches iff its distance —
l2, or minus the dot product — is finite and below x; matches in id order, the row cut to `capacity` and padded."""
import numpy as np

import bf_range_ref
import rerank_f16_ref
import rerank_pool_ref

U64MAX, NAN_BITS = bf_range_ref.U64MAX, rerank_pool_ref.NAN_BITS


def stored_rows(x, raw):
    """(the rows as they are attached, the attach's dtype argument, the f32 rows the scorer sees) for raw "f32" | "f16" | "bf16\""""
    x = np.ascontiguousarray(x, np.float32)
    bits = x if raw == "f32" else rerank_f16_ref.round_to(x, raw)
    return (x, None, x) if raw == "f32" else (bits, raw, rerank_f16_ref.widen(bits, raw))


def row(prep, q, wide, r, x, capacity=None, allowed=None, d=None, full=None):
    """(ids u64 [capacity], exact score bits u32 [capacity], total, candidates) for one query; capacity None: complete, unpadded.
    d / full: the query's estimates / exact scores of every vector where the caller has them already"""
    cand = bf_range_ref.row(prep, q, r, None, allowed, d)[0]
    score = rerank_pool_ref.exact_scores(q, wide, cand, prep.metric) if full is None else full[cand.astype(np.int64)]
    dist = score if prep.metric == 0 else -score
    with np.errstate(invalid="ignore"):
        m = np.isfinite(dist) & (dist < np.float32(x))
    ids, bits = cand[m], score[m].view(np.uint32)
    n = len(ids) if capacity is None else capacity
    out_ids, out_bits, c = np.full(n, U64MAX, np.uint64), np.full(n, NAN_BITS, np.uint32), min(len(ids), n)
    out_ids[:c], out_bits[:c] = ids[:c], bits[:c]
    return out_ids, out_bits, len(ids), len(cand)
