"""Range search restated over the CPU oracle: the reference's loop over the probed lists (search_cluster_v2_batched,
src/ivf.rs:2013-2127) with `distk` replaced by a constant R and no heap.  Probe lists and their order are the oracle's own
(`select_probes`), g_add / g_error its `probe_geometry`, and every vector's lower bound and distance its `list_vectors`, which
runs the code ref_search runs per block under the active numeric variant (`oracle.variant`).  Nothing here is taken from the
library under test."""
import numpy as np

import oracle

F32 = np.float32
PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
PAD_SCORE_BITS = 0x7FC00000


def internal_radius(metric, radius):
    """R: the caller's radius bounds the distance for L2 and the score for inner product; both are `distance < R`."""
    r = F32(radius)
    return r if metric == 0 else -r


def probed_vectors(built, q, nprobe):
    """One query -> per probed, non-empty list in probe order: (ids u64, lower bounds f32 with the reference's replacement of a
    non-finite one (:2031-2042), distances f32), each in list order"""
    metric, ex_bits = int(built.header.metric), int(built.header.ex_bits)
    rqv = oracle.rotate(built, q)
    qc = oracle.query_precompute(rqv, ex_bits)
    out = []
    for cid in oracle.select_probes(built, rqv, nprobe):
        ids = np.asarray(built.list_ids(cid), np.uint64)
        if len(ids) == 0:
            continue
        g_add, g_err = oracle.probe_geometry(built, rqv, cid)
        v = oracle.list_vectors(built, rqv, cid, g_add, g_err)
        lb = v["lb"].astype(F32).copy()
        bad = ~np.isfinite(lb)
        if bad.any():
            with np.errstate(invalid="ignore", over="ignore"):
                lb[bad] = F32(0.0) if metric == 0 else -(F32(-g_add) + F32(qc.query_norm))
        out.append((ids, lb, v["dist"].astype(F32)))
    return out


def range_query(built, q, radius, nprobe, allowed=None):
    """One query -> (ids u64, scores f32, (estimated, skipped_by_lower_bound, extended_evaluations)); matches in scan order:
    probe order, then position inside the list.  `allowed`: None, or a set-like of ids (the filter)."""
    metric, ex_bits = int(built.header.metric), int(built.header.ex_bits)
    R = internal_radius(metric, radius)
    out_i, out_s = [], []
    est = skipped = ext = 0
    for ids, lb, d in probed_vectors(built, q, nprobe):
        keep = np.ones(len(ids), bool) if allowed is None else np.fromiter((int(i) in allowed for i in ids), bool, len(ids))
        with np.errstate(invalid="ignore"):
            skip = keep & (lb >= R)  # (a NaN bound, and any bound against a NaN radius, is never skipped)
            evald = keep & ~skip
            fin = evald & np.isfinite(d)
            match = fin & (d < R)
        skipped += int(skip.sum())
        ext += int(evald.sum()) if ex_bits > 0 else 0
        est += int(fin.sum())
        out_i.append(np.asarray(ids, np.uint64)[match])
        out_s.append(d[match] if metric == 0 else -d[match])
    ids = np.concatenate(out_i) if out_i else np.zeros(0, np.uint64)
    sc = np.concatenate(out_s).astype(F32) if out_s else np.zeros(0, F32)
    return ids, sc, (est, skipped, ext)


def range_batch(built, queries, radius, nprobe, allowed=None):
    """[(ids, scores, counters)] per query"""
    return [range_query(built, q, radius, nprobe, allowed) for q in np.ascontiguousarray(queries, dtype=F32)]


def rows(ref, cap):
    """What the library returns for these reference results at capacity `cap`: (ids [nq, cap], score bits [nq, cap], totals)."""
    nq = len(ref)
    ids = np.full((nq, cap), PAD_ID, np.uint64)
    bits = np.full((nq, cap), PAD_SCORE_BITS, np.uint32)
    tot = np.zeros(nq, np.uint32)
    for q, (i, s, _) in enumerate(ref):
        k = min(len(i), cap)
        ids[q, :k] = i[:k]
        bits[q, :k] = s[:k].view(np.uint32)
        tot[q] = len(i)
    return ids, bits, tot


def diag_of(ref):
    return np.array([r[2] for r in ref], np.uint64).reshape(len(ref), 3)


def kth_distance_radius(built, q, k, nprobe):
    """The caller's radius whose internal R is the bits of query q's k-th (1-based) top-k distance with nprobe lists: the k - 1
    nearer vectors match when the distances are distinct."""
    rc, ids, sc, cnt, _ = oracle.search_batch(built, q[None, :], k, nprobe)
    assert rc == 0 and cnt[0] == k
    return F32(sc[0, k - 1])  # (score = distance for L2 and -distance for IP: exactly the caller's radius)
