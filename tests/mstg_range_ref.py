"""NumPy restatement of the MSTG range search (include/ext/rbq_mstg_range.h, rbq_mstg_range_batch) over the CPU oracle,
and the case its tests share.  No GPU.  The lists are select_lists_cpu's; every (list, position) estimate is the oracle's own
(mstg_refine_ref.candidates: the per-block code of the oracle's posting scan, in list order then vector order, nothing dropped);
the contract's steps 2 to 5 are then applied literally."""
import numpy as np

import closure_cases as cc
import mstg_refine_ref as mref
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi

NONE64, U32_MAX, DISTINCT_MAX, NAN_BITS = mref.NONE64, 0xFFFFFFFF, _abi.MSTG_RANGE_DISTINCT_MAX, 0x7FC00000


def estimates(case, q, ef, eps):
    """(lists, counts, [(ids u64, reported estimate f32) per query, scan order, the dropped candidates gone])"""
    lists, counts = rq.select_lists_cpu(q, case.c, ef, eps)
    out = []
    for i in range(len(q)):
        ids, est, _ = mref.candidates(case.built, case.pair_vec, q[i], lists[i], counts[i])
        ids, est = ids[np.isfinite(est)], est[np.isfinite(est)].astype(np.float32)  # a non-finite estimate drops the candidate
        if case.metric == 0:
            est = np.where(est > 0, est, np.float32(0)).astype(np.float32)  # distance.max(0.0)
        out.append((ids, est))
    return lists, counts, out


def range_rows(cands, radius, distinct, cap):
    """(ids [nq][cap], score bits [nq][cap], counts [nq] u32, raw totals [nq]) of the call"""
    nq = len(cands)
    ids, bits = np.full((nq, cap), NONE64, np.uint64), np.full((nq, cap), NAN_BITS, np.uint32)
    cnt, raw = np.zeros(nq, np.uint32), np.zeros(nq, np.int64)
    for i, (cid, est) in enumerate(cands):
        with np.errstate(invalid="ignore"):
            m = est < np.float32(radius)                         # (never true against a NaN radius)
        cid, est = cid[m], est[m]
        raw[i] = len(cid)
        if distinct:
            if len(cid) > DISTINCT_MAX:
                cnt[i] = U32_MAX
                continue
            o = np.lexsort((np.arange(len(cid)), est, cid))      # (id, estimate by value, scan rank)
            head = np.ones(len(o), bool)
            head[1:] = cid[o][1:] != cid[o][:-1]
            keep = np.sort(o[head])                              # back in scan order
            cid, est = cid[keep], est[keep]
        k = min(len(cid), cap)
        ids[i, :k], bits[i, :k], cnt[i] = cid[:k], est[:k].view(np.uint32), len(cid)
    return ids, bits, cnt, raw


def kth_estimate_radius(cands, k=20):
    """the median over the queries of the k-th smallest estimate (queries with fewer candidates left out)"""
    kth = [np.sort(est)[k - 1] for _, est in cands if len(est) >= k]
    return np.float32(np.median(np.asarray(kth, np.float32)))


def main_case(metric, dim, bits=3):
    """3000 rows in 48 lists (lengths no multiple of 32), closure epsilon 2.0 with max_replicas 4: 2600 clustered rows around 46
    Lloyd centroids, 400 in a tight blob around a centroid of its own (one long list: more matches than a tile of the scan holds),
    and a centroid behind the blob's that wins no row (an empty list).  16 queries a little off data points, the last of them in
    the blob, and one far outside the data, for which dynamic_prune keeps every list: more matches than the distinct limit."""
    x, c = cc.clustered(2600, dim, 46, 700 + dim)
    rng = np.random.default_rng(701 + dim)
    scale = np.float32(np.linalg.norm(x - x.mean(0), axis=1).mean())
    u = rng.standard_normal(dim).astype(np.float32)
    u /= np.linalg.norm(u)
    c_blob = (x.mean(0) + 3 * scale * u).astype(np.float32)
    blob = (c_blob + 0.01 * scale / np.sqrt(dim) * rng.standard_normal((400, dim))).astype(np.float32)
    c_empty = (c_blob + 0.5 * scale * u).astype(np.float32)     # behind the blob, seen from the data: no row is nearest to it
    x = np.concatenate([x, blob])
    c = np.concatenate([c, c_blob[None], c_empty[None]]).astype(np.float32)
    case = mref.Case(x, c, bits, metric, 2.0, 4)
    near = (x[rng.integers(0, 2600, 15)] + 0.01 * scale / np.sqrt(dim) * rng.standard_normal((15, dim))).astype(np.float32)
    far = (x.mean(0) - 40 * scale * u).astype(np.float32)
    q = np.concatenate([near, blob[:1] + np.float32(1e-3), far[None]]).astype(np.float32)
    return case, q
