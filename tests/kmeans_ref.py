"""numpy restatement of the pinned k-means (csrc/host/rbq_build.cpp, rbq_build_kmeans_faiss), written from reference
src/kmeans.rs: f32 loops vectorised over rows and clusters, sequential over coordinates, the xoshiro256** Rng of the builder."""
import numpy as np

M64 = (1 << 64) - 1


class Rng:
    """splitmix64-seeded xoshiro256** (rbq_build.cpp's Rng)."""

    def __init__(self, seed):
        z, self.s = seed & M64, []
        for _ in range(4):
            z = (z + 0x9E3779B97F4A7C15) & M64
            x = z
            x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
            x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
            self.s.append(x ^ (x >> 31))

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & M64

    def next(self):
        s = self.s
        r = (self._rotl((s[1] * 5) & M64, 7) * 9) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t  # noqa: E702
        s[3] = self._rotl(s[3], 45)
        return r


def shuffle(v, rng):
    for i in range(len(v) - 1, 0, -1):
        j = rng.next() % (i + 1)
        v[i], v[j] = v[j], v[i]


def norms(x):
    s = np.zeros(x.shape[0], np.float32)
    for j in range(x.shape[1]):
        s = s + x[:, j] * x[:, j]
    return s


def assign(x, nx, cent, block=256):
    """(best cluster u32 [rows], its distance f32 [rows]): strict < in ascending cluster order from +inf."""
    nc = norms(cent)
    best = np.zeros(x.shape[0], np.uint32)
    bestd = np.full(x.shape[0], np.inf, np.float32)
    for r0 in range(0, x.shape[0], block):
        xb = x[r0:r0 + block]
        dot = np.zeros((xb.shape[0], cent.shape[0]), np.float32)
        for j in range(x.shape[1]):
            dot = dot + xb[:, j:j + 1] * cent[None, :, j]
        d = (nx[r0:r0 + block, None] + nc[None, :]) - np.float32(2.0) * dot
        d = np.where(d < 0, np.float32(0.0), d)
        bd, bc = bestd[r0:r0 + block], best[r0:r0 + block]
        for c in range(cent.shape[0]):  # ascending cluster order, strict <
            m = d[:, c] < bd
            bd[m] = d[m, c]
            bc[m] = c
    return best, bestd


def run_kmeans(data, k, niter=25, nredo=1, seed=42, spherical=False, max_points_per_centroid=256,
               decode_block_size=32768):
    """-> (centroids [k][dim] f32, assignments [n] u32, objective float, stats {empty_reseeded, rng_draws})."""
    data = np.ascontiguousarray(data, np.float32)
    n, dim = data.shape
    sampling = Rng(seed)
    target = max(min(n, k * max_points_per_centroid), k)
    if target == n:
        x = data
    else:
        idx = list(range(n))
        shuffle(idx, sampling)
        x = data[np.sort(np.array(idx[:target], np.int64))]
    rows = x.shape[0]
    nx, full_nx = norms(x), norms(data)
    stats = {"empty_reseeded": 0, "rng_draws": 0}
    best = None
    for r in range(nredo):
        rng = Rng((seed + r * 0x9E3779B97F4A7C15) & M64)
        idx = list(range(rows))
        shuffle(idx, rng)
        cent = x[np.array(idx[:k], np.int64)].copy()
        for _ in range(niter):
            a, bd = assign(x, nx, cent)
            counts = np.bincount(a, minlength=k)
            sums = np.zeros((k, dim), np.float32)
            for i in range(rows):  # ascending row order per (cluster, coordinate)
                sums[a[i]] = sums[a[i]] + x[i]
            keys = (bd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(rows, dtype=np.uint64))
            pool = []
            for s0 in range(0, rows, decode_block_size):
                pool += sorted(keys[s0:s0 + decode_block_size].tolist(), reverse=True)[:8]
            pool.sort(reverse=True)
            nxt = 0
            for c in range(k):
                if counts[c] > 0:
                    inv = np.float32(1.0) / np.float32(counts[c])
                    cent[c] = sums[c] * inv
                else:
                    if nxt < len(pool):
                        src = 0xFFFFFFFF - (pool[nxt] & 0xFFFFFFFF)
                        nxt += 1
                    else:
                        src = rng.next() % rows
                        stats["rng_draws"] += 1
                    stats["empty_reseeded"] += 1
                    cent[c] = x[src]
            if spherical:
                nrm = norms(cent)
                for c in range(k):
                    if nrm[c] > 0:
                        cent[c] = cent[c] * (np.float32(1.0) / np.sqrt(nrm[c]))
        fin, _ = assign(data, full_nx, cent)
        delta = (data - cent[fin]).astype(np.float64)
        per_row = np.zeros(n, np.float64)
        for j in range(dim):
            per_row = per_row + delta[:, j] * delta[:, j]
        obj = 0.0
        for v in per_row.tolist():
            obj += v
        if best is None or obj < best[2]:
            best = (cent.copy(), fin.copy(), obj)
    return best[0], best[1], best[2], stats
