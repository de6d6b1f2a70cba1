"""The exact brute-force top-k with the pool chosen by rank (rbq_bf_search_exact_ranked_batch) restated per
query: the candidates are the vectors the filter lets through whose estimate (bf_ref.distances) is finite; the pool is the first
P = max(pool, top_k) of them by (total-order key of the estimate's f32 bits, id) — numpy.lexsort, no heap; from there on exactly
what tests/bf_rerank_ref.py does: rerank_pool_ref.exact_scores against bf_range_exact_ref.stored_rows' widened rows, entries whose
distance is not finite dropped, the rest ordered by (distance + 0.0, id), cut and padded."""
import numpy as np

import bf_ref
import rerank_pool_ref

U64MAX, NAN_BITS = rerank_pool_ref.PAD_ID, rerank_pool_ref.NAN_BITS


def pool_ids(prep, q, P, allowed=None):
    """the pool's ids (u64, in pool order) for one query"""
    d = bf_ref.distances(prep, q).astype(np.float32)
    keep = np.isfinite(d) if allowed is None else np.isfinite(d) & allowed
    cand = np.nonzero(keep)[0]
    return cand[np.lexsort((cand, rerank_pool_ref.total_key(d[cand])))][:P].astype(np.uint64)


def row(prep, q, wide, top_k, pool=None, allowed=None):
    """(ids u64 [top_k], exact score bits u32 [top_k], count, pool count) for one query"""
    ids = pool_ids(prep, q, max(pool or top_k, top_k), allowed)
    score = rerank_pool_ref.exact_scores(q, wide, ids, prep.metric)
    dist = score if prep.metric == 0 else -score
    keep = np.nonzero(np.isfinite(dist))[0]
    order = sorted(keep, key=lambda r: (float(dist[r] + np.float32(0.0)), int(ids[r])))[:top_k]
    out_ids, out_bits = np.full(top_k, U64MAX, np.uint64), np.full(top_k, NAN_BITS, np.uint32)
    out_ids[:len(order)], out_bits[:len(order)] = ids[order], score.view(np.uint32)[order]
    return out_ids, out_bits, len(order), len(ids)


def rows(prep, queries, wide, top_k, pool=None, allowed=None):
    """the batch: ((ids [nq, top_k] u64, score bits [nq, top_k] u32, counts [nq] u32), pool counts [nq])"""
    per = [row(prep, q, wide, top_k, pool, allowed) for q in queries]
    return tuple(np.array([p[k] for p in per], t) for k, t in enumerate((np.uint64, np.uint32, np.uint32))), np.array([p[3] for p in per])
