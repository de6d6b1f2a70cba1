"""Seeded near-ties at the scale of the shortlist scans' eps, for tests/test_gpu_gemm_shortlist_bound.py: rows whose two
nearest centroids differ in distance by a gap drawn uniformly from [-4 eps, 4 eps], every other centroid far behind.  A front
end whose |A - canonical| exceeds eps would lose the true nearest centroid of such rows; clustered test data never asks.

  pair       centroids come as close pairs b +- h v (placed at random positions); a row sits near b, shifted along v
  bisector   uncorrelated centroids; a row lies on the bisecting plane of a centroid and its nearest neighbour centroid,
             shifted along their difference (a GEMM error common to both does not cancel as it does for a close pair)

With u the unit vector from c1 to c2, L = |c2 - c1| and x = (c1 + c2) / 2 + w + t u, w orthogonal to u:
|x - c1|^2 - |x - c2|^2 = 2 t L, so t = gap / (2 L).  eps is the caller's (eps_of(Dp, span), gemm_shortlist_bound.py) at the
row's own span |x|^2 + max |c|^2.  Rows are kept only if, in float64 over the f32 values, the pair is the two nearest and the
third nearest lies more than 8 eps behind them; the tests assert their own conditions on the canonical f32 distances."""
import numpy as np

f32 = np.float32
CONFIGS = [(96, 600, 1.0), (7, 300, 1.0), (160, 514, 1e3), (960, 1024, 1e-3)]  # (dim, k, scale)
N_ROWS = 384
GENERATORS = ("pair", "bisector")


def _d2(x, c):
    """float64 squared distances [n][k] of f32 operands (the cancellation costs about 2^-50 of |x|^2 + |c|^2: nothing next to eps)"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T), 0.0)


def _rows(rng, cent, i1, i2, wscale, eps_of, Dp, n):
    """Candidate rows for the centroid pairs (i1[j], i2[j]); the first n that pass the float64 screen."""
    c = cent.astype(np.float64)
    c1, c2 = c[i1], c[i2]
    L = np.linalg.norm(c2 - c1, axis=1)
    u = (c2 - c1) / L[:, None]
    w = rng.standard_normal(c1.shape) * (wscale / np.sqrt(c1.shape[1]))
    w -= (w * u).sum(1, keepdims=True) * u
    m = (c1 + c2) / 2 + w
    ncmax = (c * c).sum(1).max()
    g = rng.uniform(-4.0, 4.0, len(i1))
    x = m
    for _ in range(3):  # (eps depends on the row's own norm, which the shift moves a little)
        eps = eps_of(Dp, ((x.astype(f32).astype(np.float64) ** 2).sum(1) + ncmax).astype(f32)).astype(np.float64)
        x = m + (g * eps / (2.0 * L))[:, None] * u
    x = x.astype(f32)
    d = _d2(x, cent)
    order = np.argsort(d, axis=1)[:, :3]
    two = np.sort(order[:, :2], axis=1)
    ok = (two == np.sort(np.stack([i1, i2], 1), axis=1)).all(1)
    if cent.shape[0] > 2:
        r = np.arange(len(x))
        ok &= d[r, order[:, 2]] - d[r, order[:, 1]] > 8.0 * eps
    keep = np.nonzero(ok)[0][:n]
    assert keep.size == n, f"only {keep.size} of {len(x)} candidate rows pass the screen"
    return x[keep]


def pair(dim, k, scale, eps_of, Dp, seed, n=N_ROWS):
    """(centroids [k][dim], rows [n][dim]) f32.  The half separation h |v| of a pair is sqrt(eps) at a typical span, so that
    the largest shift, 4 eps / (4 h |v|), is as long as the pair is wide."""
    rng = np.random.default_rng(seed)
    npairs = k // 2
    base = rng.standard_normal((k - npairs, dim)) * scale  # (k odd: the last base stays single)
    v = rng.standard_normal((npairs, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    span = 2.0 * dim * scale * scale
    h = np.sqrt(float(eps_of(Dp, f32(span))))
    cent = np.concatenate([base[:npairs] + h * v, base[:npairs] - h * v, base[npairs:]])
    perm = rng.permutation(k)  # the members of a pair sit anywhere: other lanes, other tiles
    where = np.empty(k, np.int64)
    where[perm] = np.arange(k)
    cent = cent[perm].astype(f32)
    j = np.arange(3 * n) % npairs
    return cent, _rows(rng, cent, where[j], where[j + npairs], 0.1 * scale, eps_of, Dp, n)


def bisector(dim, k, scale, eps_of, Dp, seed, n=N_ROWS):
    """(centroids [k][dim], rows [n][dim]) f32: uncorrelated Gaussian centroids."""
    rng = np.random.default_rng(seed)
    cent = (rng.standard_normal((k, dim)) * scale).astype(f32)
    d = _d2(cent, cent)
    np.fill_diagonal(d, np.inf)
    nn = d.argmin(1)
    i1 = rng.permutation(np.arange(6 * n) % k)
    return cent, _rows(rng, cent, i1, nn[i1], 0.05 * scale, eps_of, Dp, n)


def make(gen, dim, k, scale, eps_of, Dp, seed):
    return {"pair": pair, "bisector": bisector}[gen](dim, k, scale, eps_of, Dp, seed)


def tie_stats(C, eps):
    """From canonical distances C [n][k] and eps [n]: (share of rows whose two nearest lie within 2 eps, rows with a third
    centroid within 4 eps of the nearest, mask of the near-tie rows, the two nearest centroids [n][2])."""
    C = np.asarray(C, np.float64)
    order = np.argsort(C, axis=1, kind="stable")[:, :3]
    r = np.arange(C.shape[0])
    near = C[r, order[:, 1]] - C[r, order[:, 0]] <= 2.0 * eps
    third = (C[r, order[:, 2]] - C[r, order[:, 0]] <= 4.0 * eps) if C.shape[1] > 2 else np.zeros(len(r), bool)
    return float(near.mean()), np.nonzero(third)[0], near, order[:, :2]
