"""Inputs of the scan-instantiation sweep (tests/test_scan_instantiation_cases_host.py on the CPU, tests/test_gpu_scan_instantiations.py
on the GPU): one recipe per (dim, bits, metric), small enough to run at every compile-time instantiation of
k_scanw and k_scan, and shaped so that every call of the sweep has ties inside the top-k, tie-free rows, vectors skipped by the
lower bound and more refined candidates than results.
* 2400 base vectors from six Gaussian components (0.35 sigma noise), assigned round-robin; the first 150 vectors of component 0
  appended twice more: exact triplicates, bit-identical distances;
* 12 lists, FHT-Kac rotator; inner-product data and queries normalised;
* 48 queries: the first 24 triplicated vectors themselves (their rows contain ties), and 24 vectors of components 3 to 5 plus
  0.03 sigma noise (their rows are tie-free);
* nprobe 6; top_k on both sides of every register-class boundary of both kernels (k_scanw: < 64, < 128, <= 255; k_scan: <= 63,
  64..128, 129..256); one filtered call (every third id) at top_k 10 and one at top_k 100."""
import functools

import numpy as np

from conftest import build_index

DIMS = (128, 256, 384, 512, 768, 960, 1024, 1536)  # the compile-time dimensions of k_scanw / k_scan
BITS = (1, 3, 7)                                    # total bits: ex_bits 0, 2, 6
METRICS = (0, 1)                                    # L2, inner product
TOP_KS = (10, 63, 64, 127, 128, 129, 255, 256)
FILTERED_TOP_KS = (10, 100)
NPROBE = 6
NLIST = 12
N_COMP, N_BASE, N_DUP, SIGMA = 6, 2400, 150, 0.35
N = N_BASE + 2 * N_DUP
NQ_DUP, NQ_FAR = 24, 24
NQ = NQ_DUP + NQ_FAR


def seed(dim, bits):
    return 52000 + 8 * dim + bits


def _normalised(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=4)
def case(dim, bits, metric):
    """(data [N][dim], built index, queries [NQ][dim]) of one (dim, bits, metric)"""
    rng = np.random.default_rng(seed(dim, bits))
    means = rng.standard_normal((N_COMP, dim)).astype(np.float32)
    comp = np.arange(N_BASE) % N_COMP
    base = (means[comp] + SIGMA * rng.standard_normal((N_BASE, dim)).astype(np.float32)).astype(np.float32)
    if metric == 1:
        base = _normalised(base)
    dup = base[comp == 0][:N_DUP]
    data = np.ascontiguousarray(np.concatenate([base, dup, dup]), dtype=np.float32)  # every row of dup exists three times
    far_src = rng.choice(np.nonzero(comp >= 3)[0], NQ_FAR, replace=False)
    far = base[far_src] + np.float32(0.03) * rng.standard_normal((NQ_FAR, dim)).astype(np.float32)
    if metric == 1:
        far = _normalised(far)
    q = np.ascontiguousarray(np.concatenate([dup[:NQ_DUP], far]), dtype=np.float32)
    _, built = build_index(nlist=NLIST, total_bits=bits, metric=metric, rotator=1, seed=seed(dim, bits), data=data, dim=dim)
    return data, built, q


def filter_words():
    """the dense id filter of the filtered calls: every third id allowed"""
    allowed = np.arange(0, N, 3)
    words = np.zeros((N + 31) // 32, np.uint32)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    return words, N
