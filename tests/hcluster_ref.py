"""NumPy restatement of MSTG's hierarchical balanced clustering (csrc/host/rbq_hcluster.hpp, rbq_build_hcluster), written from
reference src/mstg/clustering.rs on top of tests/kmeans_ref.py: every f32 operation one NumPy f32 operation, no code shared
with the C++."""
import numpy as np

import kmeans_ref

F32 = np.float32


def l2_distance_sqr(a, b):
    """math::l2_distance_sqr in the order an AVX2 host takes: 8 accumulators over whole groups of 8, summed from -0.0, then
    the tail one by one (src/math.rs:216-245)."""
    n = a.shape[0]
    main = n // 8 * 8
    s = F32(0.0)
    if main:
        acc = np.zeros(8, F32)
        for i in range(0, main, 8):
            d = a[i:i + 8] - b[i:i + 8]
            acc = acc + d * d
        s = F32(-0.0)
        for lane in range(8):
            s = F32(s + acc[lane])
    for i in range(main, n):
        d = F32(a[i] - b[i])
        s = F32(s + F32(d * d))
    return s


def l2_rows(x, c):
    """l2_distance_sqr(row, c) for every row of x, the same order, vectorised over the rows."""
    n = x.shape[1]
    main = n // 8 * 8
    s = np.zeros(x.shape[0], F32)
    if main:
        acc = np.zeros((x.shape[0], 8), F32)
        for i in range(0, main, 8):
            d = x[:, i:i + 8] - c[None, i:i + 8]
            acc = acc + d * d
        s = np.full(x.shape[0], -0.0, F32)
        for lane in range(8):
            s = s + acc[:, lane]
    for i in range(main, n):
        d = x[:, i] - c[i]
        s = s + d * d
    return s


def max_allowed(target, w):
    """(target as f32 * (1.0 + w)) as usize, Rust's saturating cast."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = F32(F32(target) * F32(F32(1.0) + F32(w)))
    if np.isnan(v) or v <= 0:
        return 0
    if v >= F32(2.0 ** 64):
        return (1 << 64) - 1
    return int(v)


def centroid(x):
    s = np.zeros(x.shape[1], F32)
    for i in range(x.shape[0]):
        s = s + x[i]
    return s / F32(x.shape[0])


class Stuck(Exception):
    """A split left one non-empty subcluster: the crate would never end."""


def cluster(data, max_cluster_size, k, balance_weight, max_iterations=100):
    """-> (centroids [count][dim] f32, offsets [count + 1] u64, members [n] u32, stats)."""
    data = np.ascontiguousarray(data, F32)
    n, dim = data.shape
    rng = kmeans_ref.Rng(42)
    stats = {"splits": 0, "balance_moves": 0, "empty_reseeded": 0, "rng_draws": 0}
    stack, final = [list(range(n))], []
    w = F32(balance_weight)
    while stack:
        rows = stack.pop()
        if len(rows) <= max_cluster_size:
            final.append(rows)
            continue
        seed = rng.next()
        x = data[np.array(rows, np.int64)]
        cent, asg, _, st = kmeans_ref.run_kmeans(x, k, niter=max_iterations, nredo=1, seed=seed, spherical=False,
                                                 max_points_per_centroid=256, decode_block_size=32768)
        stats["splits"] += 1
        stats["empty_reseeded"] += st["empty_reseeded"]
        stats["rng_draws"] += st["rng_draws"]
        sub = [[] for _ in range(k)]
        for i, c in enumerate(asg.tolist()):
            sub[c].append(rows[i])
        if w > 0:
            target = len(rows) // k
            limit = max_allowed(target, w)
            for _ in range(10):
                sizes = [len(s) for s in sub]
                over = next((i for i, s in enumerate(sizes) if s > limit), None)
                under = next((i for i, s in enumerate(sizes) if s < target), None)
                if over is None or under is None:
                    break
                d = l2_rows(data[np.array(sub[over], np.int64)], cent[under])
                best, bd = 0, d[0]
                for i in range(1, len(d)):
                    if d[i] < bd:
                        best, bd = i, d[i]
                sub[under].append(sub[over].pop(best))
                stats["balance_moves"] += 1
        sub = [s for s in sub if s]
        if len(sub) < 2:
            raise Stuck()
        stack += sub
    cents = np.stack([centroid(data[np.array(rows, np.int64)]) for rows in final])
    offsets = np.cumsum([0] + [len(r) for r in final]).astype(np.uint64)
    members = np.array([i for r in final for i in r], np.uint32)
    return cents, offsets, members, stats
