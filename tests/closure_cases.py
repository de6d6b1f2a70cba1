"""Inputs of the closure-assignment tests (tests/test_closure_host.py on the CPU, tests/test_gpu_mstg_build.py on the GPU): the
four input sets of closure.rs's own unit tests, seeded clustered data, and tie-heavy sets."""
import numpy as np

import rabitq_rs_amd as rq
from conftest import make_dataset

EPSILONS = (0.0, 0.15, 2.0, 10.0)
REPLICAS = (1, 3, 8, 16)

# (epsilon, max_replicas, vectors, centroids) of src/mstg/closure.rs:114-189
CRATE_UNIT = [
    (0.2, 8, [[0.1, 0.0]], [[0.0, 0.0]]),
    (0.5, 8, [[0.1, 0.0], [0.5, 0.0]], [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [2.0, 0.0]]),
    (2.0, 8, [[0.25, 0.0]], [[0.0, 0.0], [0.5, 0.0], [1.0, 0.0], [0.0, 0.5]]),
    (10.0, 3, [[0.25, 0.0]], [[0.0, 0.0], [0.1, 0.0], [0.2, 0.0], [0.3, 0.0], [0.4, 0.0], [0.5, 0.0]]),
]


def clustered(n, dim, k, seed, intrinsic=3, noise=0.02):
    """make_dataset in `intrinsic` dimensions, embedded in `dim` with a little noise, and k Lloyd centroids: few intrinsic
    dimensions put many vectors near the boundary of several clusters."""
    low = make_dataset(n, intrinsic, 64, seed)
    rng = np.random.default_rng(seed + 1)
    proj = rng.standard_normal((intrinsic, dim)).astype(np.float32) / np.float32(np.sqrt(intrinsic))
    x = (low @ proj + noise * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    cent, _ = rq.builder.kmeans(x, k, 5, seed)
    return x, cent


def main_case():
    """The main seeded case: 800 vectors, dim 128, 40 centroids, epsilon 2 (the value closure.rs's own RNG-rule test uses; at
    MSTG's default 0.15 Gaussian-mixture data replicates only a few percent of its vectors), max_replicas 8."""
    x, c = clustered(800, 128, 40, 11)
    return x, c, 2.0, 8


def uniform_cloud(n, dim, k, seed, intrinsic=10, lloyd=1):
    """uniform data in an `intrinsic`-dimensional cube, embedded in `dim`, and k centroids after `lloyd` iterations: a large
    share of a cell's volume lies near its faces, so vectors replicate even within a small epsilon."""
    low = make_dataset(n, intrinsic, 1, seed, uniform=True)
    rng = np.random.default_rng(seed + 1)
    proj = rng.standard_normal((intrinsic, dim)).astype(np.float32) / np.float32(np.sqrt(intrinsic))
    x = (low @ proj + 0.005 * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    cent, _ = rq.builder.kmeans(x, k, lloyd, seed)
    return x, cent


def default_epsilon_case():
    """A second seeded case at the crate's default epsilon 0.15 and max_replicas 8.  The RNG rule itself trims what the small
    threshold lets through, so this data replicates less than the main case: its condition is a replication of at least 1.1."""
    x, c = uniform_cloud(800, 64, 30, 13)
    return x, c, 0.15, 8


def shortlist_dim_cases():
    """name -> (data, centroids) with more than 256 centroids (the device's GEMM shortlist path) at dims below 8, not a multiple
    of 8, and not a multiple of 32"""
    return {"d7_k260": clustered(500, 7, 260, 51), "d9_k300": clustered(500, 9, 300, 52), "d100_k300": clustered(500, 100, 300, 53)}


def dim_cases():
    """name -> (data, centroids): dims 7, 8, 9, 100, 128; n_lists 1, below max_replicas, well above it."""
    out = {}
    for dim, k in ((7, 12), (8, 40), (9, 5), (100, 40), (128, 1), (128, 3)):
        out["d%d_k%d" % (dim, k)] = clustered(240, dim, k, 100 + dim + k)
    return out


def tie_cases():
    out = {}
    x, c = clustered(200, 16, 10, 5)
    out["duplicated_centroids"] = (x, np.concatenate([c, c[::2], c[:3]]).astype(np.float32))
    x, c = clustered(120, 9, 12, 6)
    xe = x.copy()
    xe[:12] = c  # vectors equal to a centroid: the closest distance and the threshold are 0
    out["vector_equals_centroid"] = (xe, np.concatenate([c, c[:4]]).astype(np.float32))
    rng = np.random.default_rng(9)
    out["integer_grid"] = (rng.integers(-2, 3, (200, 10)).astype(np.float32), rng.integers(-2, 3, (30, 10)).astype(np.float32))
    return out
