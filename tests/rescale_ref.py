"""best_rescale_factor (reference src/quantizer.rs:337-427) restated in plain Python with heapq, and the crafted inputs
the CPU and GPU tests feed it.  Python floats are IEEE f64 and `/` and math.sqrt round correctly, so the restatement is
bit-exact: it is the yardstick for both the CPU builder's export and the GPU kernel (k_rescale.hip)."""
import heapq
import math
import sys

import numpy as np

K_TIGHT_START = [0.0, 0.15, 0.20, 0.52, 0.59, 0.71, 0.75, 0.77, 0.81]
K_EPS, K_NENUM = 1e-5, 10.0


def best_rescale_factor(o_abs, ex_bits):
    o = [float(v) for v in np.asarray(o_abs, np.float32)]
    dim = len(o)
    max_o = max([0.0] + o)
    if max_o <= sys.float_info.epsilon:
        return 1.0
    t_end = (((1 << ex_bits) - 1) + K_NENUM) / max_o
    t_start = t_end * K_TIGHT_START[min(ex_bits, 8)]
    cur = [int(t_start * v + K_EPS) for v in o]
    sqr_den, num = dim * 0.25, 0.0
    for c, v in zip(cur, o):
        sqr_den += float(c * c + c)
        num += (c + 0.5) * v
    heap = [((cur[i] + 1) / o[i], i) for i in range(dim) if o[i] > 0.0]
    heapq.heapify(heap)
    max_ip, best_t = 0.0, t_start
    while heap:
        t, i = heapq.heappop(heap)
        if t >= t_end:
            continue
        cur[i] += 1
        u = cur[i]
        sqr_den += 2.0 * u
        num += o[i]
        ip = num / math.sqrt(sqr_den)
        if ip > max_ip:
            max_ip, best_t = ip, t
        if u < (1 << ex_bits) - 1 and o[i] > 0.0:
            tn = (u + 1) / o[i]
            if tn < t_end:
                heapq.heappush(heap, (tn, i))
    if best_t <= 0.0:
        return max(t_start, sys.float_info.epsilon)
    return best_t


def normalize(g):
    """o = |g| / norm(g) in f32, norm the sequential f32 chain of the encoder; clipped to 1 (f32 rounding of a one-hot)."""
    g = np.abs(np.asarray(g, np.float32))
    n2 = np.float32(0.0)
    for v in g:
        n2 = np.float32(n2 + np.float32(v * v))
    norm = np.float32(np.sqrt(n2))
    if norm == 0:
        return g
    return np.minimum(g / norm, np.float32(1.0)).astype(np.float32)


def normalize_rows(G):
    """normalize() for many rows at once (np.sum's pairwise order: fine for test inputs, o only has to be in [0, 1])."""
    G = np.abs(np.asarray(G, np.float32))
    norm = np.sqrt((G * G).sum(axis=1, dtype=np.float32)).astype(np.float32)
    norm[norm == 0] = 1.0
    return np.minimum(G / norm[:, None], np.float32(1.0)).astype(np.float32)


def crafted_rows(dim, seed):
    """(name, o) pairs covering the sweep's corners: Gaussian, near-constant magnitudes (most events per vector), duplicated
    magnitudes (t ties across coordinates), one-hot, zeros, a single dominant coordinate, all zero."""
    rng = np.random.default_rng(seed)
    out = [("gauss", normalize(rng.standard_normal(dim))),
           ("near_const", normalize(1.0 + 1e-3 * rng.standard_normal(dim))),
           ("exact_const", normalize(np.ones(dim))),
           ("dup4", normalize(rng.integers(1, 5, dim).astype(np.float32))),
           ("dup2_halfzero", normalize(rng.integers(0, 2, dim) * rng.choice([1.0, 3.0], dim))),
           ("one_hot", normalize(np.eye(dim, dtype=np.float32)[dim // 3])),
           ("zeros", normalize(rng.standard_normal(dim) * (rng.random(dim) < 0.3))),
           ("peaked", normalize(np.r_[[40.0], rng.standard_normal(dim - 1) * 0.01])),
           ("two_level", normalize(np.where(rng.random(dim) < 0.5, 1.0, 1.0 + 2.0 ** -20))),
           ("all_zero", np.zeros(dim, np.float32))]
    return out
