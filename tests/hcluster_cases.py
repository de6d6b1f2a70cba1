"""Inputs of the hierarchical-clustering tests (tests/test_hcluster_host.py, tests/test_gpu_hcluster.py): the smallest shapes that
reach each path of rbq_mstg_cluster_device.  A case is (data, max_posting_size, branching_factor, balance_weight,
max_iterations)."""
import functools

import numpy as np


def _uniform(n, dim, seed):
    return np.random.default_rng(seed).random((n, dim), dtype=np.float32)


def _blob(n, dim, seed):
    """70 % of the rows in one tight blob, the rest spread out: k-means leaves one subcluster far over the balance limit."""
    rng = np.random.default_rng(seed)
    tight = int(n * 0.7)
    x = np.concatenate([rng.normal(0.0, 0.01, (tight, dim)), rng.uniform(-4.0, 4.0, (n - tight, dim))]).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(n)])


def _identical(n, dim):
    return np.tile(np.linspace(0.25, 1.0, dim, dtype=np.float32), (n, 1))


@functools.lru_cache(maxsize=None)
def cases():
    c = {
        "crate_basic_100x8": (_uniform(100, 8, 12345), 20, 4, 1.0, 8),
        "crate_balance_1000x32": (_uniform(1000, 32, 12345), 100, 5, 1.0, 8),
        "sampled_1500x16_k4": (_uniform(1500, 16, 3), 100, 4, 1.0, 6),
        "sampled_600x16_k2": (_uniform(600, 16, 4), 100, 2, 1.0, 6),
        "balancing_600x8": (_blob(600, 8, 5), 60, 4, 0.25, 8),
        "identical_50_k4": (_identical(50, 8), 20, 4, 1.0, 6),
        "identical_60_k12": (_identical(60, 8), 11, 12, 1.0, 6),
        "gemm_3000x32_k300": (_uniform(3000, 32, 6), 299, 300, 1.0, 3),
    }
    for d in (1, 7, 13, 33):
        c[f"odd_dim_{d}"] = (_uniform(400, d, 100 + d), 40, 3, 1.0, 6)
    return c


SAMPLED = "sampled_1500x16_k4"
BALANCING = "balancing_600x8"
IDENTICAL = ("identical_50_k4", "identical_60_k12")


@functools.lru_cache(maxsize=None)
def cpu(name):
    """The CPU restatement's result on a case, computed once: (centroids, offsets, members, stats)."""
    import rabitq_rs_amd as rq
    x, mps, k, w, it = cases()[name]
    return rq.hierarchical_cluster_cpu(x, mps, k, w, it)


def same(a, b):
    """Two results agree in every array, bit for bit (stats apart)."""
    assert a[0].shape == b[0].shape, (a[0].shape, b[0].shape)
    assert np.array_equal(a[1], b[1]), "offsets differ"
    assert np.array_equal(a[2], b[2]), "members differ"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "centroids differ"
