"""The GPU encoder in the optimal-rescale mode (RabitqConfig::new: every vector's own best_rescale_factor, searched by
k_rescale.hip) against the CPU builder's train_with_clusters(..., use_faster_config=False): the per-vector t bit for bit,
then every device array of the index byte for byte, one-shot and streamed, and the search results against the oracle."""
import struct

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import make_dataset
from rescale_ref import crafted_rows, normalize, normalize_rows
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu


def _same_index(ref, enc, hdr, nlist):
    D, ex = hdr.padded_dim, hdr.ex_bits
    Dc = (D + 63) // 64 * 64
    ln = ref.debug_copy_index("list_n", np.empty(nlist, np.uint32))
    nblocks = int(((ln + 31) // 32).sum())
    cpu_u = 128 // ex if ex else 1
    w4 = ((D // 16 + cpu_u - 1) // cpu_u) if ex else 0
    sizes = {"list_gb0": nlist * 4, "list_n": nlist * 4, "centroids": nlist * D * 4, "blocks": nblocks * (Dc * 4 + 384),
             "ids": nblocks * 32 * 8, "bsum": nblocks * 32}
    if ex:
        sizes.update({"ex": nblocks * 32 * w4 * 256, "fadd_ex": nblocks * 32 * 4, "fres_ex": nblocks * 32 * 4})
    for name, nbytes in sizes.items():
        a = ref.debug_copy_index(name, np.empty(nbytes, np.uint8))
        b = enc.debug_copy_index(name, np.empty(nbytes, np.uint8))
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at {bad[:5]}"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. per-vector t -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex_bits", [2, 6])
@pytest.mark.parametrize("dim", [64, 128, 960, 2048])
def test_device_best_rescale_matches_cpu(dim, ex_bits):
    rows = [o for _, o in crafted_rows(dim, 77 * dim + ex_bits)]
    rng = np.random.default_rng(dim * 10 + ex_bits)
    nrand = 10000 if dim <= 960 else 2000
    O = np.concatenate([np.stack(rows), normalize_rows(rng.standard_normal((nrand, dim)))])
    if dim == 2048:  # near-constant magnitudes: ~18 k events per vector, far more than one LDS window holds
        O = np.concatenate([O, normalize_rows(1.0 + 1e-3 * rng.standard_normal((64, dim)))])
    got = rq.IvfRabitqIndex.debug_best_rescale(O, ex_bits)
    want = np.array([rq.builder.best_rescale_factor(o, ex_bits) for o in O])
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: gpu {got[bad[:3]]} cpu {want[bad[:3]]}"


def test_device_best_rescale_ties_and_other_widths():
    """exact ties across coordinates (equal magnitudes) settle by coordinate index; ex 1 starts at the top code"""
    for ex_bits in (1, 3, 7):
        O = np.stack([o for _, o in crafted_rows(320, 5 + ex_bits)] + [normalize(np.ones(320))])
        got = rq.IvfRabitqIndex.debug_best_rescale(O, ex_bits)
        want = np.array([rq.builder.best_rescale_factor(o, ex_bits) for o in O])
        assert np.array_equal(_bits(got), _bits(want)), ex_bits


# ---- 2. one-shot build -----------------------------------------------------------------------------------------------
ENC_CASES = [
    # n, dim, nlist, bits, metric, rotator
    pytest.param(6000, 960, 40, 7, 0, 1, id="opt_d960_7bit_L2"),
    pytest.param(5000, 960, 40, 3, 1, 1, id="opt_d960_3bit_IP"),
    pytest.param(4000, 100, 24, 7, 0, 1, id="opt_d100_pad128_7bit_L2"),
    pytest.param(4000, 128, 32, 1, 0, 1, id="opt_d128_1bit_L2"),
    pytest.param(3000, 48, 24, 3, 0, 0, id="opt_matrix_d48_3bit_L2"),
    pytest.param(3000, 64, 20, 7, 1, 0, id="opt_matrix_d64_7bit_IP"),
    pytest.param(2500, 2048, 16, 7, 0, 1, id="opt_d2048_7bit_L2"),
]


@pytest.mark.parametrize("n,dim,nlist,bits,metric,rot", ENC_CASES)
def test_optimal_device_encoder_matches_cpu_builder(n, dim, nlist, bits, metric, rot):
    import torch
    data = make_dataset(n, dim, max(nlist // 4, 1), 341, normalize=(metric == 1))
    cent, assign = rq.builder.kmeans(data, nlist, 5, 342)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rot, 343, False)
    ref = rq.IvfRabitqIndex.from_built(built)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    enc = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, None, rescale="optimal")
    _same_index(ref, enc, built.hdr, nlist)
    q = make_dataset(32, dim, max(nlist // 4, 1), 344, normalize=(metric == 1))
    _compare(built, enc, q, 10, min(8, nlist))
    ref.close(); enc.close()


# ---- 3. streamed build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,nlist,bits,metric,rot", [
    pytest.param(7000, 960, 40, 7, 0, 1, id="stream_opt_d960_7bit_L2"),
    pytest.param(5000, 100, 24, 3, 1, 1, id="stream_opt_d100_pad128_3bit_IP"),
    pytest.param(3000, 64, 20, 7, 1, 0, id="stream_opt_matrix_d64_7bit_IP"),
])
def test_optimal_stream_builder_matches_one_shot(n, dim, nlist, bits, metric, rot):
    import torch
    data = make_dataset(n, dim, max(nlist // 4, 1), 441, normalize=(metric == 1))
    cent, assign = rq.builder.kmeans(data, nlist, 5, 442)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rot, 443, False)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    one = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, rescale="optimal")
    sizes = np.bincount(assign, minlength=nlist).astype(np.uint32)
    sb = rq.StreamBuilder(built.hdr_ptr, cent, sizes, None, rescale="optimal")
    cuts = [0, 1, 700, 701, n // 2, n - 13, n]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k % 2 == 0:
            sb.push(data[a:b], assign[a:b], a)
        else:  # device pointers
            sb.push(xd[a:b].contiguous().data_ptr(), ad[a:b].contiguous().data_ptr(), a, b - a)
    enc = sb.finish()
    _same_index(one, enc, built.hdr, nlist)
    ref = rq.IvfRabitqIndex.from_built(built)
    _same_index(ref, enc, built.hdr, nlist)
    ref.close(); one.close(); enc.close()


# ---- 4. Python convenience -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("faster", [False, True])
def test_train_on_device_matches_cpu_build(faster):
    import torch
    n, dim, nlist = 5000, 200, 32
    data = make_dataset(n, dim, 8, 541)
    cent, assign = rq.builder.kmeans(data, nlist, 4, 542)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 543, faster)
    ref = rq.IvfRabitqIndex.from_built(built)
    enc = rq.IvfRabitqIndex.train_on_device(data, cent, assign, 7, 0, 1, 543, faster)
    _same_index(ref, enc, built.hdr, nlist)
    enc.close()
    enc = rq.IvfRabitqIndex.train_on_device(torch.from_numpy(data).cuda(), cent, torch.from_numpy(assign.astype(np.int64)).cuda(),
                                            7, 0, 1, 543, faster)
    _same_index(ref, enc, built.hdr, nlist)
    ref.close(); enc.close()


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------
def test_optimal_with_one_bit_equals_const():
    import torch
    n, dim, nlist = 3000, 128, 16
    data = make_dataset(n, dim, 4, 641)
    cent, assign = rq.builder.kmeans(data, nlist, 3, 642)
    built = rq.builder.train_with_clusters(data, cent, assign, 1, 0, 1, 643, True)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    a = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, built.t_const)
    b = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, None, rescale="optimal")
    _same_index(a, b, built.hdr, nlist)
    a.close(); b.close()


def test_unknown_rescale_mode_is_invalid_config():
    import torch
    n, dim, nlist = 2000, 64, 8
    data = make_dataset(n, dim, 2, 741)
    cent, assign = rq.builder.kmeans(data, nlist, 3, 742)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 743, True)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    for mode in ("best", 2, -1):
        with pytest.raises(rq.RabitqError) as e:
            rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, built.t_const, rescale=mode)
        assert e.value.kind == "InvalidConfig"
        with pytest.raises(rq.RabitqError) as e:
            rq.StreamBuilder(built.hdr_ptr, cent, np.bincount(assign, minlength=nlist), built.t_const, rescale=mode)
        assert e.value.kind == "InvalidConfig"
    with pytest.raises(rq.RabitqError) as e:  # the constant mode still needs its factor
        rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, None, rescale="const")
    assert e.value.kind == "InvalidConfig"
    with pytest.raises(rq.RabitqError) as e:  # o outside [0, 1]
        rq.IvfRabitqIndex.debug_best_rescale(np.full((2, 16), 2.0, np.float32), 6)
    assert e.value.kind == "InvalidConfig"


def test_optimal_large_d960_7bit_matches_cpu():
    import torch
    n, dim, nlist = 50000, 960, 64
    rng = np.random.default_rng(841)
    data = (rng.standard_normal((n, dim), dtype=np.float32) + 0.3 * rng.standard_normal((1, dim), dtype=np.float32))
    assign = rng.integers(0, nlist, n).astype(np.uint32)
    cent = np.stack([data[assign == c].mean(axis=0) for c in range(nlist)]).astype(np.float32)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 843, False)
    ref = rq.IvfRabitqIndex.from_built(built)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    enc = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, rescale="optimal")
    _same_index(ref, enc, built.hdr, nlist)
    ref.close(); enc.close()
