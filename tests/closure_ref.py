"""NumPy restatement of MSTG's closure assignment, written from the crate's text (src/mstg/closure.rs:24-107 and
math::l2_distance_sqr's AVX2 body, src/math.rs:216-245).  It shares no code with the library: the tests hold the CPU
restatement (rbq_build_closure_assign) and the device (rbq_mstg_closure_assign) against it.  Every operation is an f32
operation with one rounding, in the crate's order."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)
f32 = np.float32


def l2_rows(x, cents):
    """l2_distance_sqr(x, c) for every row c of cents: 8 accumulators over the whole chunks of 8 coordinates, their sum in lane
    order, then the tail coordinates one by one."""
    x = np.asarray(x, f32)
    cents = np.asarray(cents, f32)
    k, dim = cents.shape
    chunks = dim // 8
    total = np.zeros(k, f32)
    if chunks:
        acc = np.zeros((k, 8), f32)
        for i in range(chunks):
            d = (x[None, 8 * i:8 * i + 8] - cents[:, 8 * i:8 * i + 8]).astype(f32)
            acc = (acc + (d * d).astype(f32)).astype(f32)
        for lane in range(8):
            total = (total + acc[:, lane]).astype(f32)
    for j in range(chunks * 8, dim):
        d = (x[j] - cents[:, j]).astype(f32)
        total = (total + (d * d).astype(f32)).astype(f32)
    return total


def assign_one(x, cents, epsilon, max_replicas, info=None):
    """ClosureAssigner::assign: the crate's Vec of cluster indices.  `info`, when a dict, receives `order` (the stable order's
    first max_replicas entries), `candidates` (those within the threshold) and `removed` (what the RNG rule dropped)."""
    dist = l2_rows(x, cents)
    order = np.argsort(dist, kind="stable")          # sort_by(partial_cmp): stable, equal distances keep ascending index
    closest = dist[order[0]]
    threshold = f32(closest * f32(f32(1.0) + f32(epsilon)))   # closest_dist * (1.0 + epsilon): the sum is rounded first
    head = order[:max_replicas]
    cand = [int(c) for c in head if dist[c] <= threshold]
    kept = []
    for c in cand:
        ok = True
        for s in kept:
            pair = l2_rows(cents[s], cents[c:c + 1])[0]  # l2_distance_sqr(c_selected, c_candidate)
            if dist[c] > pair:
                ok = False
                break
        if ok:
            kept.append(c)
    if cand[0] not in kept:
        kept.insert(0, cand[0])
    if info is not None:
        info.update(order=[int(c) for c in head], candidates=cand, removed=len(cand) - len(kept))
    return kept


def closure_assign(data, cents, epsilon, max_replicas, stats=None):
    """(lists [n][max_replicas] u32 with UINT32_MAX in unused slots, counts [n] u32).  `stats`, when a dict, receives
    `removed` [n] (candidates dropped by the RNG rule) and `order` [n] lists."""
    data = np.ascontiguousarray(data, f32)
    cents = np.ascontiguousarray(cents, f32)
    n = data.shape[0]
    lists = np.full((n, max_replicas), NONE, np.uint32)
    counts = np.zeros(n, np.uint32)
    removed = np.zeros(n, np.int64)
    orders = []
    for i in range(n):
        info = {}
        kept = assign_one(data[i], cents, epsilon, max_replicas, info)
        lists[i, :len(kept)] = kept
        counts[i] = len(kept)
        removed[i] = info["removed"]
        orders.append(info["order"])
    if stats is not None:
        stats.update(removed=removed, order=orders)
    return lists, counts
