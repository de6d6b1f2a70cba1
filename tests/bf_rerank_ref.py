"""The exact brute-force top-k (rbq_bf_search_exact_batch) restated per query: the pool is bf_ref.search at
top_k := P = max(pool, top_k) — the authority on which estimates are in it, ties included; every entry is scored by
rerank_pool_ref.exact_scores (the oracle's canonical sums) against bf_range_exact_ref.stored_rows' widened rows; entries whose
distance — l2, or minus the dot product — is not finite are dropped; the rest is ordered by (distance + 0.0, id), cut and padded."""
import numpy as np

import bf_ref
import rerank_pool_ref

U64MAX, NAN_BITS = rerank_pool_ref.PAD_ID, rerank_pool_ref.NAN_BITS


def row(prep, q, wide, top_k, pool=None, allowed=None):
    """(ids u64 [top_k], exact score bits u32 [top_k], count, pool count) for one query"""
    ids = bf_ref.search(prep, q, max(pool or top_k, top_k), allowed)[0]
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
