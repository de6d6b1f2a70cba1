"""BruteForceRabitqIndex.train_on_device (rbq_bf_train_device) against the CPU builder: the RBF1 stream of a device-trained
index equals, byte for byte, the stream of the index uploaded from builder.train_bruteforce for the same input.  RBF1 holds
every array of the index (sign codes, ex codes, the eight factor arrays), so stream equality is array-for-array bit equality.
The reference is always the CPU builder, never the device path itself."""
import ctypes as C

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import bruteforce as bfm
from rabitq_rs_amd.index import _check
import bf_ref

pytestmark = pytest.mark.gpu
BF = rq.BruteForceRabitqIndex


def cpu_bytes(data, bits, metric, rotator, seed, faster):
    built = rq.builder.train_bruteforce(data, bits, metric, rotator, seed, faster)
    idx = BF.from_built(built)
    try:
        return idx.save_to_bytes()
    finally:
        idx.close()
        built.close()


def dev_bytes(data, bits, metric, rotator, seed, faster, **kw):
    idx = BF.train_on_device(data, bits, metric, rotator, seed, faster, **kw)
    try:
        assert len(idx) == data.shape[0] and idx.dim == data.shape[1]
        return idx.save_to_bytes()
    finally:
        idx.close()


def first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d / %d" % (len(a), len(b))
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    d = np.flatnonzero(x != y)
    return "%d bytes differ, first at %d of %d" % (d.size, d[0], len(a)) if d.size else "equal"


def gaussian(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
@pytest.mark.parametrize("rotator,dim", [(1, 128), (1, 100), (1, 960), (0, 32), (0, 48)],
                         ids=["fht-128", "fht-100", "fht-960", "matrix-32", "matrix-48"])
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_matrix(bits, metric, rotator, dim, faster):
    data = gaussian(3000, dim, 1000 * bits + 10 * dim + metric)  # 3000: not a multiple of 32, 64 or 256
    seed = 7 + bits + dim
    want, got = cpu_bytes(data, bits, metric, rotator, seed, faster), dev_bytes(data, bits, metric, rotator, seed, faster)
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("n", [1, 31, 33, 257, 50000])
def test_sizes(n):
    data = gaussian(n, 128, n)
    want, got = cpu_bytes(data, 7, 0, 1, n, True), dev_bytes(data, 7, 0, 1, n, True)
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
def test_chunking_does_not_change_the_index(faster):
    """the encoder's tile is 64 rows: chunks of 1 and 37 rows end inside a tile"""
    data = gaussian(1500, 192, 5)
    want = cpu_bytes(data, 7, 1, 1, 5, faster)
    for chunk in (0, 1, 37, 1024):
        got = dev_bytes(data, 7, 1, 1, 5, faster, max_chunk_rows=chunk)
        assert got == want, (chunk, first_difference(got, want))


def test_input_kinds():
    """a host array, a CUDA tensor, and a raw device pointer through the C entry"""
    import torch
    data = gaussian(2100, 100, 8)
    want = cpu_bytes(data, 3, 0, 1, 21, False)
    assert dev_bytes(data, 3, 0, 1, 21, False) == want
    xd = torch.from_numpy(data).cuda()
    assert dev_bytes(xd, 3, 0, 1, 21, False) == want
    assert dev_bytes(torch.from_numpy(data), 3, 0, 1, 21, False) == want  # (a CPU tensor is a host array)
    small = rq.builder.train_bruteforce(data[:1], 3, 0, 1, 21, True)
    for rescale, t_const, ref in ((rq._abi.RESCALE_OPTIMAL, 0.0, want), (rq._abi.RESCALE_CONST, small.t_const, cpu_bytes(data, 3, 0, 1, 21, True))):
        h = C.c_void_p()
        _check(bfm.lib().rbq_bf_train_device(C.cast(small.hdr_ptr, C.c_void_p), xd.data_ptr(), 2100, rescale, t_const, 500, -1, C.byref(h)))
        idx = BF(h)
        assert idx.save_to_bytes() == ref
        idx.close()


def special_rows(dim, rotator, seed):
    """one data set with the rows that exercise every guard of quantize_with_centroid against the zero centroid"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((200, dim)).astype(np.float32)
    x[3] = 0.0                                   # norm <= eps: left uncoded, every dot a signed zero
    x[4] = -0.0
    x[10] = x[2]; x[11] = x[2]; x[150] = x[2]    # exact duplicates
    x[20] = 1e-3; x[20, 7] = 1e3                 # one component 1e6 times the rest
    x[21, :] = 1.0; x[21, dim - 1] = -1e6
    x[30] = np.float32(1e-40)                    # denormals
    x[31] = (rng.standard_normal(dim) * 1e-39).astype(np.float32)
    x[40] = np.float32(1e-9)                     # |<r, xu_cb>| <= eps and norm <= eps
    x[41] = np.float32(3e-8) * np.sign(rng.standard_normal(dim)).astype(np.float32)  # norm > eps at dim >= 16
    if rotator == 0:  # Matrix: rows whose rotation is (nearly) one axis of 2e-7: norm > eps while <r, xu_cb> ~ 1e-7 <= eps
        built = rq.builder.train_bruteforce(x[:1], 7, 0, 0, seed, True)
        m = np.frombuffer(built.rotator_blob(), np.float32).reshape(dim, dim)
        x[50] = np.float32(2e-7) * m[0, :]
        x[51] = np.float32(2e-7) * m[:, 0]
        x[52] = np.float32(-2.2e-7) * m[5, :]
        x[53] = np.float32(-2.2e-7) * m[:, 5]
        built.close()
    else:
        x[50] = 0.0
        x[50, 0] = 2e-7
    return x


@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("rotator,dim", [(1, 128), (0, 32), (1, 64)], ids=["fht-128", "matrix-32", "fht-64"])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_special_vectors(bits, rotator, dim, metric, faster):
    data = special_rows(dim, rotator, 77)
    want, got = cpu_bytes(data, bits, metric, rotator, 77, faster), dev_bytes(data, bits, metric, rotator, 77, faster)
    assert got == want, first_difference(got, want)
    if rotator == 0 and bits == 7:  # the data set does reach the guards it is meant for
        a = rq.builder.train_bruteforce(data, bits, metric, rotator, 77, faster).arrays()
        assert a["residual_norm"][3] == 0 and a["f_rescale"][3] == 0 and not a["ex"][3].any()
        tiny = [i for i in (50, 51, 52, 53) if a["residual_norm"][i] > np.finfo(np.float32).eps and a["f_rescale"][i] == 0]
        assert tiny, "no row with a coded residual and |<r, xu_cb>| <= eps"


def test_large_optimal_at_dim_1024():
    data = gaussian(20000, 1024, 99)
    want, got = cpu_bytes(data, 7, 0, 1, 99, False), dev_bytes(data, 7, 0, 1, 99, False)
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
def test_a_device_trained_index_searches_like_the_cpu_trained_one(metric):
    data = gaussian(4000, 128, 31)
    data[2000:2400] = data[:400]  # equal distances: the heap's tie path
    built = rq.builder.train_bruteforce(data, 7, metric, 1, 31, False)
    cpu, dev = BF.from_built(built), BF.train_on_device(data, 7, metric, 1, 31, False)
    prep = bf_ref.Prepared(built.hdr_ptr, built.arrays())
    q = gaussian(64, 128, 32)
    for k in (10, 1000):
        a, b = cpu.batch_search_raw(q, rq.BruteForceSearchParams(k)), dev.batch_search_raw(q, rq.BruteForceSearchParams(k))
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        for i in (0, 17, 63):
            rid, rsc = bf_ref.search(prep, q[i], k)
            assert b[2][i] == len(rid) and np.array_equal(b[0][i, :len(rid)], rid)
            assert np.array_equal(b[1][i, :len(rid)].view(np.uint32), rsc.view(np.uint32))
    allowed = list(range(0, 4000, 7))
    fa = cpu.search_filtered(q[5], rq.BruteForceSearchParams(50), allowed)
    fb = dev.search_filtered(q[5], rq.BruteForceSearchParams(50), allowed)
    mask = np.zeros(4000, bool)
    mask[allowed] = True
    rid, rsc = bf_ref.search(prep, q[5], 50, mask)
    assert fa == fb and [r.id for r in fb] == [int(i) for i in rid]
    assert np.array_equal(np.array([r.score for r in fb], np.float32).view(np.uint32), rsc.view(np.uint32))


@pytest.mark.parametrize("bits", [3, 7])
def test_save_and_load(bits):
    data = gaussian(900, 100, bits)
    dev = BF.train_on_device(data, bits, 1, 1, 3, True)
    blob = dev.save_to_bytes()
    loaded = BF.load_from_bytes(blob)
    assert len(loaded) == 900 and loaded.save_to_bytes() == blob
    q = gaussian(12, 100, 1)
    a, b = dev.batch_search_raw(q, rq.BruteForceSearchParams(20)), loaded.batch_search_raw(q, rq.BruteForceSearchParams(20))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_one_bit_stream_is_refused_on_load_as_for_a_cpu_trained_index():
    data = gaussian(300, 128, 2)
    blob = dev_bytes(data, 1, 0, 1, 2, True)
    assert blob == cpu_bytes(data, 1, 0, 1, 2, True)
    with pytest.raises(rq.RabitqError, match="checksum mismatch"):
        BF.load_from_bytes(blob)


def test_determinism():
    data = gaussian(5000, 256, 4)
    assert dev_bytes(data, 7, 0, 1, 4, False) == dev_bytes(data, 7, 0, 1, 4, False)
    assert dev_bytes(data, 3, 1, 1, 4, True) == dev_bytes(data, 3, 1, 1, 4, True)
