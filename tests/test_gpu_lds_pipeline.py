"""k_scanw's staged ex dot product (scan_codes.hpp: `ex_dot_one_regs<.., AHEAD>`, the query values requested one or two stretches of
four codes ahead) and its lookups at the edges of their stages, not at the workload's shape.

The lookups run over the code dwords of a vector, four per 128-column granule and two in the 64-column tail; the ex dot is
pipelined over stretches of four codes across the code units' boundaries.  A staged loop goes wrong in its first and its last
stage, so the cases are the granule counts at the edges: 128 (one granule), 256 (two), 384 (three, an odd count), 960 (seven and
the tail), 1024 (eight, no tail), 1536 (twelve) — each at 1 bit (no ex dot), 3 bits (ex_bits 2: one code unit per lane, 8 to 96 codes)
and 7 bits (ex_bits 6: one to four or more units, 8 to 96 codes, the last stretch and the last unit partly filled), at top_k 10 and
100 (TR = 1 and 2: the single and the paired dot product).  D = 192 is the runtime-dimension kernel, whose path does not change.
n = 4000 in 16 lists, all probed, 128 queries: the batch size from which the device entry picks k_scanw by itself.

Every case is `_both_kernels` of test_gpu_round5: ids, scores, counts and the diagnostics counters against the oracle, with and
without diagnostics, and k_scanw against k_scan bit for bit."""
import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import build_index, make_dataset
from test_gpu_round5 import _both_kernels

pytestmark = pytest.mark.gpu

N, NLIST, NPROBE, NQ = 4000, 16, 16, 128
DIMS = (128, 256, 384, 960, 1024, 1536)
BITS = (1, 3, 7)

_built = {}


def _index(dim, bits):
    """one index per (dim, bits), shared by the cases that use it and never changed"""
    if (dim, bits) not in _built:
        _built[(dim, bits)] = build_index(n=N, dim=dim, nlist=NLIST, total_bits=bits, seed=7100 + dim + bits)
    return _built[(dim, bits)]


def _queries(data, dim, seed):
    """half far from the data (few survivors per tile: short rounds), half beside indexed vectors (full rounds)"""
    rng = np.random.default_rng(seed)
    far = make_dataset(NQ // 2, dim, 4, seed + 1)
    near = data[rng.choice(data.shape[0], NQ - NQ // 2, replace=False)] + 0.03 * rng.standard_normal((NQ - NQ // 2, dim)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([far, near]), dtype=np.float32)


@pytest.mark.parametrize("top_k", (10, 100))
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("dim", DIMS)
def test_staged_loops_at_the_granule_edges(dim, bits, top_k):
    data, built = _index(dim, bits)
    idx = rq.IvfRabitqIndex.from_built(built)
    _both_kernels(built, idx, _queries(data, dim, 7200 + dim), top_k, NPROBE)
    idx.close()


@pytest.mark.parametrize("top_k", (10, 100))
def test_runtime_dimension_kernel_is_unchanged(top_k):
    data, built = _index(192, 7)
    idx = rq.IvfRabitqIndex.from_built(built)
    _both_kernels(built, idx, _queries(data, 192, 7250), top_k, NPROBE)
    idx.close()


def test_staged_loops_under_a_filter():
    """D = 960 at 7 bits (seven granules and the tail, three code units) with every third id allowed"""
    data, built = _index(960, 7)
    idx = rq.IvfRabitqIndex.from_built(built)
    allowed = np.arange(0, N, 3)
    words = np.zeros((N + 31) // 32, np.uint32)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    _both_kernels(built, idx, _queries(data, 960, 7300), 10, NPROBE, words, N)
    idx.close()


def test_staged_loops_twice_per_query_on_tie_heavy_data():
    """Exact duplicates inside the top-k: the query restarts on the exact heap and goes through the lookups and the dot products a
    second time (D = 256 at 7 bits: two granules, and a dot product with its query values requested ahead; at 384 the dot product is
    the plain one)."""
    base = make_dataset(N - 500, 256, 4, 7400)
    data = np.concatenate([base, base[:500]], axis=0)
    _, built = build_index(nlist=NLIST, total_bits=7, data=data, dim=256)
    idx = rq.IvfRabitqIndex.from_built(built)
    q = np.ascontiguousarray(np.concatenate([base[:NQ // 2], make_dataset(NQ // 2, 256, 4, 7401)]))
    r0 = idx.heap_restarts()
    _both_kernels(built, idx, q, 10, NPROBE)
    assert idx.heap_restarts() - r0 >= NQ // 2  # the duplicated neighbours did restart their queries
    idx.close()
