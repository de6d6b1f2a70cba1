"""The ranking GEMM reads ONE image per operand, hi | lo interleaved per 32-element K slab (csrc/device/hl_layout.hpp), with every
wave-level load covering whole 128-byte lines.  Nothing in the arithmetic moves, so every case holds
  (a) the raw images ("cent_hl", "rot_hl") to the interleave of bf16_split of the centroids / rotated queries, and the logical views
      ("cent_hi" / "cent_lo", "rot_hi" / "rot_lo") to the planes themselves, bit for bit;
  (b) the score rows to the GEMM's float64 budget (tests/rank_bound.py);
  (c) without split-K, the score rows to those of the SAME kernel on planar copies of the operands (debug option rank_planar), bit
      for bit (with split-K the order of the atomic additions is free: only (b));
  (d) for one shape per tile and metric, ids, counts and scores to the oracle's.
Shapes: D 64 (two slabs: split-K 4 leaves two parts without one), 192 (six slabs: 3 + 3, and 2 + 2 + 2 + 0) and 960 (the headline's
30: 15 + 15, and 8 + 8 + 8 + 6); 129 and 1000 lists, 1 / 127 / 129 / 1025 queries: ragged tile edges in both directions and clamped rows in every tile
of 64, 128 and 128 x 256.  The three kernels that write the query image are all reached: k_prep_wave (1 and 1025 queries), the
latency front as a preparation (127) and k_prep (129, option wg_prep)."""
import numpy as np
import pytest

import rank_bound as rb
from test_gpu_parity import RTOL, _compare
from test_gpu_rank_bound import TOP_K, _Case, _device_search, _queries, _rank_workgroups, _set, _tiles
from test_rank_lines_host import interleave

pytestmark = pytest.mark.gpu

DIMS = [64, 192, 960]
NLISTS = [129, 1000]
NQS = [1, 127, 129, 1025]
TILES = [64, 128, 256]
NPROBE = 16


@pytest.fixture(scope="module")
def env():
    import torch
    cache = {}
    stream = torch.cuda.Stream(torch.device("cuda", 0))

    def get(dim, nlist, metric):
        k = (dim, nlist, metric)
        if k not in cache:
            case = _Case(dim, nlist, metric, 1, "mix")  # (its constructor holds "cent_hi" / "cent_lo" to bf16_split(centroids))
            assert case.D == dim
            hl = case.idx.debug_copy_index("cent_hl", np.empty((nlist, 2 * dim), np.uint16))
            assert np.array_equal(hl, interleave(*rb.bf16_split(case.cent))), "cent_hl differs from the interleave of bf16_split(centroids)"
            cache[k] = case
        return cache[k]
    yield get, stream
    for c in cache.values():
        c.close()


def _prep_opts(nq):
    """Which kernel prepares the queries (all of them write the image): see the module docstring."""
    if nq == 127:
        return {"latency_path": 1}
    if nq == 129:
        return {"latency_path": 0, "wg_prep": 1}
    return {"latency_path": 0}


def _call(case, stream, q, nq, planar):
    """One device call; the score rows, the rotated queries and the results."""
    case.idx.set_option("rank_planar", planar)
    ids, sc, cnt = _device_search(case, stream, q, NPROBE)
    A = case.idx.debug_copy_workspace(stream.cuda_stream, "scores", np.empty((nq, case.nlist), np.float32))
    rot = case.idx.debug_copy_workspace(stream.cuda_stream, "rot", np.empty((nq, case.D), np.float32))
    return A, rot, (ids, sc, cnt)


def _check_images(case, stream, nq, rot, what):
    D = case.D
    wh, wl = rb.bf16_split(rot)
    hl = case.idx.debug_copy_workspace(stream.cuda_stream, "rot_hl", np.empty((nq, 2 * D), np.uint16))
    assert np.array_equal(hl, interleave(wh, wl)), f"{what}: rot_hl differs from the interleave of bf16_split(rot)"
    rh = case.idx.debug_copy_workspace(stream.cuda_stream, "rot_hi", np.empty((nq, D), np.uint16))
    rl = case.idx.debug_copy_workspace(stream.cuda_stream, "rot_lo", np.empty((nq, D), np.uint16))
    assert np.array_equal(rh, wh) and np.array_equal(rl, wl), f"{what}: rot_hi / rot_lo differ from bf16_split(rot)"


def _check_budget(case, A, rot, what):
    worst, viol, _ = rb.check_rows(A, rot, case.cent, case.metric, case.D, skip_rewritten=True)
    print(f"{what}: worst |A - s64| / budget = {worst:.4f}")
    assert not viol, f"{what}: {len(viol)} score(s) outside the GEMM budget, first (q, list) {viol[0]}"


def _run(env, dim, nlist, nq, tile, metric, ksplit=1, oracle=False):
    get, stream = env
    case = get(dim, nlist, metric)
    what = f"D {dim} nlist {nlist} nq {nq} tile {tile} metric {metric} split-K {ksplit}"
    q = _queries("mix", nq, dim, 11 + nq + dim)
    opts = {"rank_tile": tile, "rank_ksplit": ksplit} if ksplit > 1 else {"rank_tile": tile, "rank_ksplit": 0, **_prep_opts(nq)}
    _set(case.idx, opts)
    try:
        # (the route the case means is the one the call launches; a part of a split without a slab still counts as a workgroup)
        assert _rank_workgroups(case.idx, nq, NPROBE) == _tiles(nlist, nq, tile) * ksplit, what
        A, rot, res = _call(case, stream, q, nq, 0)
        _check_images(case, stream, nq, rot, what)                                 # (a)
        _check_budget(case, A, rot, what)                                          # (b)
        A1, rot1, res1 = _call(case, stream, q, nq, 1)
        assert np.array_equal(rot.view(np.uint32), rot1.view(np.uint32))
        _check_images(case, stream, nq, rot1, what + " (planar)")
        if ksplit == 1:                                                            # (c)
            bad = np.nonzero((A.view(np.uint32) != A1.view(np.uint32)).any(1))[0]
            assert bad.size == 0, f"{what}: score rows of the interleaved and the planar route differ for queries {bad[:10]}"
        else:
            _check_budget(case, A1, rot1, what + " (planar)")
        for x, y in zip(res, res1):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), what
        if oracle:                                                                 # (d)
            case.idx.set_option("rank_planar", 0)
            ids, sc, cnt = res
            hids, hsc, hcnt = _compare(case.built, case.idx, q, TOP_K, NPROBE)
            assert np.array_equal(cnt, hcnt), f"{what}: device-call counts differ from the oracle's"
            bad = np.nonzero((ids != hids).any(axis=1))[0]
            assert bad.size == 0, f"{what}: device-call ids differ from the oracle's for queries {bad[:10]}"
            for i in range(nq):
                np.testing.assert_allclose(sc[i, :cnt[i]], hsc[i, :cnt[i]], rtol=RTOL, atol=0)
    finally:
        case.idx.set_option("rank_planar", 0)
        _set(case.idx, {})


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("nlist", NLISTS)
@pytest.mark.parametrize("dim", DIMS)
def test_tiles(env, dim, nlist, nq, tile, metric):
    _run(env, dim, nlist, nq, tile, metric)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("ks", [2, 4])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("nq", [127, 129])
@pytest.mark.parametrize("nlist", NLISTS)
@pytest.mark.parametrize("dim", DIMS)
def test_split_k(env, dim, nlist, nq, tile, ks, metric):
    """D 64: two slabs, so two of four parts have none; D 192: six slabs as 3 + 3 and 2 + 2 + 2 + 0; D 960: 15 + 15 and 8 + 8 + 8 + 6."""
    _run(env, dim, nlist, nq, tile, metric, ksplit=ks)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("tile", TILES)
def test_results_match_oracle(env, tile, metric):
    _run(env, 192, 1000, 129, tile, metric, oracle=True)
