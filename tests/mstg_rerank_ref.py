"""NumPy restatement of the exact rerank of the MSTG candidate pool (option "mstg_rerank" on rbq_mstg_search_refined_batch;
include/rbq_mstg.h).  No GPU.

Step 1, the pool with its ranks and the `tie_at_cut` flag, is mstg_refine_ref's (`candidates` / `binary_pool`); the canonical sums
are rerank_pool_ref.exact_scores (the oracle's ref_l2_distance_sqr / ref_dot), negated for inner product; steps 2 to 4 are
applied literally."""
import numpy as np

import mstg_refine_ref as rref
import rerank_pool_ref as pref

NONE64 = rref.NONE64


def widen_bf16(bits):
    """bf16 bit patterns (uint16) as the f32 they widen to"""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16(x):
    """f32 -> bf16 bit patterns, round to nearest even (finite input)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def distances(query, raw, ids, metric):
    """the reported distance of `query` to raw[id] for every id: canon_l2, or -canon_dot (a sign flip); NaN without a raw row"""
    s = pref.exact_scores(query, raw, ids, metric)
    return s if metric == 0 else (-s).astype(np.float32)


def rerank_query(ids, est, query, raw, metric, top_k, refine_pool, n_raw=None):
    """Steps 1 to 4 for one query over its candidates (ids, est) in (list order, vector order):
    (ids [top_k], scores [top_k], count, pool ids, tie_at_cut, number of distinct raw rows read)."""
    pool = max(int(refine_pool), int(top_k))
    n_raw = len(raw) if n_raw is None else int(n_raw)
    sel, _e, tie = rref.binary_pool(est, metric, pool)           # step 1: sel[r] = the candidate of rank r
    pid = ids[sel]
    rank = np.arange(len(sel))
    # step 2: per id the smallest rank, before any scoring; ids without a raw row leave
    o = np.lexsort((rank, pid))
    first = np.ones(len(o), bool)
    first[1:] = pid[o][1:] != pid[o][:-1]
    o = o[first]
    o = o[pid[o] < np.uint64(n_raw)]
    pid, rank = pid[o], rank[o]
    # step 3
    d = distances(query, raw[:n_raw], pid, metric)
    fin = np.isfinite(d)
    d, pid, rank = d[fin], pid[fin], rank[fin]
    # step 4: by value (-0.0 == +0.0 to the float comparison of lexsort), then rank
    o = np.lexsort((rank, d))[:top_k]
    out_ids = np.full(top_k, NONE64, np.uint64)
    out_sc = np.full(top_k, np.nan, np.float32)
    out_ids[:len(o)] = pid[o]
    out_sc[:len(o)] = d[o]
    return out_ids, out_sc, len(o), ids[sel], tie, int(len(first) and first.sum())


def rerank_ref(built, pair_vec, queries, lists, counts, raw, metric, top_k, refine_pool, cands=None, n_raw=None, wide_queries=None):
    """The whole call: ids [nq][top_k], scores, counts, and per query whether a tie sat at the pool's cut.
    `queries`: what the binary stage sees (f32); `wide_queries` (default: the same) what the exact score sees — both are the
    caller's rows widened.  `cands`: mstg_refine_ref.all_candidates of the same queries and lists."""
    q = np.ascontiguousarray(queries, np.float32)
    wq = q if wide_queries is None else np.ascontiguousarray(wide_queries, np.float32)
    raw = np.ascontiguousarray(raw, np.float32)
    nq = len(q)
    ids = np.full((nq, top_k), NONE64, np.uint64)
    sc = np.full((nq, top_k), np.nan, np.float32)
    cnt = np.zeros(nq, np.uint32)
    ties = []
    for i in range(nq):
        cid, est, _dist = cands[i] if cands is not None else rref.candidates(built, pair_vec, q[i], lists[i], counts[i])
        ids[i], sc[i], cnt[i], _p, t, _n = rerank_query(cid, est, wq[i], raw, metric, top_k, refine_pool, n_raw)
        ties.append(t)
    return ids, sc, cnt, ties
