"""GPU parity tests of k_scanw's refine rounds below top_k 64 (scanw.hpp: the instantiations whose loop of rounds requests the
next tile's records once, outside the loop) at the edges of a round.  A round takes up to four candidates, one per 16-lane group.
(Rounds of eight with the second candidate's code units staged in LDS were measured on these same cases and not kept:
profiles/scanw_pairs_lds.)
Every case: ids, scores, counts and the diagnostics counters against the oracle (`_compare`, with and without diagnostics), and
k_scanw (`scan_wave = 1`) against k_scan (`scan_wave = 0`) bit for bit (`_both_kernels`).
* the instantiations: D = 960 / 768 / 128 at 7 bits (ex_bits 6, three / three / one code unit per lane) and D = 128 at 3 bits
  (ex_bits 2), 128 queries per call (the batch size from which the device entry picks k_scanw), top_k 1, 5, 10, 63;
* the edges of a round: first tiles with exactly 3, 4, 5 and 8 candidates (lists of that many vectors probed alone: the threshold
  is infinite, every vector of the tile is wanted), lists shorter than eight vectors and shorter than top_k, tie-heavy data
  (the replay and the exact-heap restart), a filtered call, twelve streams at once;
* top_k 100 (two registers per lane: the loop of rounds as it was) beside them.
Both kernels give the same results by construction, so the results of these tests do not tell which one served a call; the
stage probe does (`stage_resources(...)["scan"]`: 64 threads and 16 bytes of scratch at the most is k_scanw, 256 threads k_scan),
and tests/test_gpu_scan_instantiations.py asserts it for every compile-time instantiation, these among them."""
import functools

import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
from conftest import build_index, make_dataset
from test_gpu_round5 import _both_kernels

pytestmark = pytest.mark.gpu

N, NLIST, NPROBE, NQ = 20000, 16, 16, 128


@functools.lru_cache(maxsize=None)
def _index(dim, bits):
    data, built = build_index(n=N, dim=dim, nlist=NLIST, total_bits=bits, seed=7100 + dim + bits)
    rng = np.random.default_rng(7101 + dim)
    far = make_dataset(NQ // 2, dim, 4, 7102)
    near = data[rng.choice(N, NQ - NQ // 2, replace=False)] + 0.03 * rng.standard_normal((NQ - NQ // 2, dim)).astype(np.float32)
    q = np.ascontiguousarray(np.concatenate([far, near]), dtype=np.float32)
    return data, built, q


@pytest.mark.parametrize("top_k", [1, 5, 10, 63])
@pytest.mark.parametrize("dim,bits", [(960, 7), (768, 7), (128, 7), (128, 3)])
def test_refine_rounds_match_oracle_and_workgroup_kernel(dim, bits, top_k):
    _, built, q = _index(dim, bits)
    idx = rq.IvfRabitqIndex.from_built(built)
    _both_kernels(built, idx, q, top_k, NPROBE)
    idx.close()


TINY = (3, 4, 5, 8)  # vectors in the tiny lists


@functools.lru_cache(maxsize=None)
def _tiny_lists_index(dim):
    """12 ordinary lists and four far-away ones of 3, 4, 5 and 8 vectors; 32 queries beside each tiny list"""
    rng = np.random.default_rng(7200 + dim)
    means = rng.standard_normal((12, dim)).astype(np.float32)
    comp = rng.integers(0, 12, 3000)
    base = means[comp] + 0.35 * rng.standard_normal((3000, dim)).astype(np.float32)
    tiny_c = (6.0 * rng.standard_normal((len(TINY), dim))).astype(np.float32)
    tiny = [tiny_c[i] + 0.2 * rng.standard_normal((c, dim)).astype(np.float32) for i, c in enumerate(TINY)]
    data = np.ascontiguousarray(np.concatenate([base] + tiny), dtype=np.float32)
    assign = np.concatenate([comp] + [np.full(c, 12 + i) for i, c in enumerate(TINY)]).astype(np.uint32)
    cent = np.ascontiguousarray(np.concatenate([means, tiny_c]), dtype=np.float32)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 7201, True)
    q = np.concatenate([tiny_c[i] + 0.1 * rng.standard_normal((NQ // len(TINY), dim)).astype(np.float32) for i in range(len(TINY))])
    return built, np.ascontiguousarray(q, dtype=np.float32)


@pytest.mark.parametrize("dim", [960, 128])
def test_first_tiles_of_three_four_five_and_eight_candidates(dim):
    """nprobe 1: the whole scan of a query is one tile of 3 / 4 / 5 / 8 candidates, all wanted (less than a round of four, exactly
    one, one more, two), short counts where the list is shorter than top_k; nprobe 2 and 16: the same first block beside the
    first block of the next list (a first tile of more than eight), then the rest."""
    built, q = _tiny_lists_index(dim)
    sizes = built.list_sizes()
    assert sorted(int(s) for s in sizes[-len(TINY):]) == sorted(TINY)
    idx = rq.IvfRabitqIndex.from_built(built)
    for nprobe in (1, 2, 16):
        for top_k in (1, 5, 10, 63):
            _, _, cnt = _both_kernels(built, idx, q, top_k, nprobe)
            if nprobe == 1:
                want = np.repeat(np.minimum(np.array(TINY), top_k), NQ // len(TINY))
                assert np.array_equal(cnt, want), "each query scans exactly its tiny list"
    idx.close()


@functools.lru_cache(maxsize=None)
def _tie_index():
    base = make_dataset(3000, 128, 6, 7300)
    dup = base[:300]
    data = np.concatenate([base, dup, dup], axis=0)  # vectors 0..299 exist three times
    _, built = build_index(nlist=16, total_bits=7, data=data, dim=128)
    return base, built


@pytest.mark.parametrize("top_k", [1, 5, 10, 63])
def test_refine_rounds_on_tie_heavy_data(top_k):
    """triplicated vectors inside the top-k (exact-heap restart) and outside it (lazy ties)"""
    base, built = _tie_index()
    idx = rq.IvfRabitqIndex.from_built(built)
    q = np.ascontiguousarray(np.concatenate([base[:64], base[1500:1564] + np.float32(0.02)]))
    _both_kernels(built, idx, q, top_k, 8)
    idx.close()


def test_refine_rounds_filtered():
    data, built, q = _index(128, 7)
    idx = rq.IvfRabitqIndex.from_built(built)
    allowed = np.arange(0, N, 3)
    words = np.zeros((N + 31) // 32, np.uint32)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    _both_kernels(built, idx, q, 10, NPROBE, words, N)
    idx.close()


def test_refine_rounds_on_twelve_streams():
    import torch
    dev = torch.device("cuda", 0)
    _, built, q = _index(960, 7)
    idx = rq.IvfRabitqIndex.from_built(built)
    top_k, ns = 10, 12
    rc, oids, _, ocnt, _ = oracle.search_batch(built, q, top_k, NPROBE)
    assert rc == 0
    qd = torch.from_numpy(q).to(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(ns)]
    d_ids = [torch.zeros(NQ, top_k, dtype=torch.int64, device=dev) for _ in range(ns)]
    d_sc = [torch.zeros(NQ, top_k, dtype=torch.float32, device=dev) for _ in range(ns)]
    d_cnt = [torch.zeros(NQ, dtype=torch.int32, device=dev) for _ in range(ns)]
    torch.cuda.synchronize(dev)
    for rep in range(6):
        for i in range(ns):
            idx.search_batch_device(qd.data_ptr(), NQ, 960, top_k, NPROBE, d_ids[i].data_ptr(), d_sc[i].data_ptr(),
                                    d_cnt[i].data_ptr(), stream=streams[i].cuda_stream)
        torch.cuda.synchronize(dev)
        for i in range(ns):
            got = d_ids[i].cpu().numpy().view(np.uint64)
            bad = np.nonzero((got != oids).any(axis=1))[0]
            assert bad.size == 0, f"rep {rep} stream {i}: ids differ for queries {bad[:10]}"
            assert np.array_equal(d_cnt[i].cpu().numpy().view(np.uint32), ocnt)
            d_ids[i].zero_()
    for st in streams:
        idx.release_stream(st.cuda_stream)
    idx.close()


def test_top_100_keeps_both_candidates_in_registers():
    _, built, q = _index(960, 7)
    idx = rq.IvfRabitqIndex.from_built(built)
    _both_kernels(built, idx, q, 100, NPROBE)
    idx.close()
