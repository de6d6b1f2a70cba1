"""Saving a device-resident IVF index as RBQ1 (rbq_index_save_rbq1*, include/rbq_persist.h; the crate's save_to_writer,
src/ivf.rs:1310-1474): the bytes against the CPU builder's writer and the independent tests/rbq1_writer.py over every
creation path, load -> save round trips of streams with odd bytes, the streamed writer, errors, and the GPU CRC-32."""
import io
import struct
import threading
import zlib

import numpy as np
import pytest

import rabitq_rs_amd as rq
import rbq1_writer
from conftest import make_dataset
from rabitq_rs_amd import _abi
from rabitq_rs_amd.index import WRITE_FN, lib
from rabitq_rs_amd.kmeans import KMeansConfig, first_draw

pytestmark = pytest.mark.gpu

# list sizes of the crafted assignment: empty lists, 1, 31, 32, 33 (one past a block) and a large one
SIZES = [0, 1, 31, 32, 33, 300, 0, 65]


def _dataset(dim, metric, seed):
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    data = make_dataset(n, dim, 4, seed, normalize=(metric == 1))
    assign = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES)).astype(np.uint32)  # lists interleaved in id order
    cent = np.stack([data[assign == c].mean(0) if s else data[c] for c, s in enumerate(SIZES)]).astype(np.float32)
    return data, cent, assign


def _same(got, want, what):
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(a.size, b.size)
    bad = np.nonzero(a[:m] != b[:m])[0]
    raise AssertionError(f"{what}: {len(got)} vs {len(want)} bytes, {bad.size} differ, first at {bad[:5]}")


def _stream_build(built, cent, data, assign, faster):
    sizes = np.bincount(assign, minlength=len(SIZES)).astype(np.uint32)
    sb = rq.StreamBuilder(built.hdr_ptr, cent, sizes, built.t_const if faster else None, rescale="const" if faster else "optimal")
    n = data.shape[0]
    for a, b in zip([0, 1, 200, n // 2], [1, 200, n // 2, n]):
        sb.push(data[a:b], assign[a:b], a)
    return sb.finish()


# ---- 1. the bytes equal the CPU writer's, for every creation path ------------------------------------------------------
# (the Matrix rotator keeps padded_dim == dim, which the device needs to be a multiple of 16: dim 100 is padded by FhtKac only)
@pytest.mark.parametrize("rot,dim", [(1, 64), (1, 100), (1, 960), (1, 2048), (0, 64), (0, 960), (0, 2048)],
                         ids=["fhtkac-64", "fhtkac-100", "fhtkac-960", "fhtkac-2048", "matrix-64", "matrix-960", "matrix-2048"])
@pytest.mark.parametrize("ex_bits", [0, 2, 6])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_save_equals_cpu_writer(metric, ex_bits, rot, dim):
    import torch
    data, cent, assign = _dataset(dim, metric, 1000 + dim + 7 * ex_bits + 3 * metric + rot)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    for faster in ((True, False) if ex_bits else (True,)):
        built = rq.builder.train_with_clusters(data, cent, assign, ex_bits + 1, metric, rot, 77 + dim, faster)
        want = built.save_rbq1()
        _same(rbq1_writer.from_built(built), want, "independent writer vs CPU writer")
        paths = {
            "load_from_bytes": lambda: rq.IvfRabitqIndex.load_from_bytes(want),
            "build_on_device": lambda: rq.IvfRabitqIndex.build_on_device(
                built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), data.shape[0], built.t_const if faster else None,
                rescale="const" if faster else "optimal"),
            "StreamBuilder": lambda: _stream_build(built, cent, data, assign, faster),
        }
        if faster:
            paths["from_built"] = lambda: rq.IvfRabitqIndex.from_built(built)
        for name, make in paths.items():
            idx = make()
            _same(idx.save_to_bytes(), want, f"{name} faster={faster}")
            idx.close()
        built.close()


@pytest.mark.parametrize("bits,metric,rot,faster", [(7, 0, 1, False), (3, 1, 1, True), (1, 0, 0, True), (7, 1, 0, True)])
def test_save_after_train_equals_cpu_writer(bits, metric, rot, faster):
    """IvfRabitqIndex.train (device k-means + encoder) against train_with_clusters over the same clustering"""
    data = make_dataset(3000, 128, 12, 31 + bits, normalize=(metric == 1))
    idx = rq.IvfRabitqIndex.train(data, 24, bits, metric, rot, 4242, faster)
    km = rq.run_kmeans_with_config(data, 24, KMeansConfig(niter=30, seed=first_draw(4242 ^ 0x5A5A5A5A5A5A5A5A)))
    built = rq.builder.train_with_clusters(data, km.centroids, km.assignments.astype(np.uint32), bits, metric, rot, 4242, faster)
    _same(idx.save_to_bytes(), built.save_rbq1(), "train")
    built.close(); idx.close()


def test_device_recon_factors_match_cpu_bitwise():
    """delta / vl on the device (rbq_debug_copy_index) against the BuiltIndex's, slot by slot"""
    import torch
    data, cent, assign = _dataset(960, 0, 5)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 9, False)
    xd, ad = torch.from_numpy(data).cuda(), torch.from_numpy(assign.astype(np.int32)).cuda()  # (held: a temporary's memory is reused)
    idx = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), data.shape[0],
                                            rescale="optimal")
    nslots = sum((s + 31) // 32 for s in SIZES) * 32
    for name in ("delta", "vl"):
        got = idx.debug_copy_index(name, np.empty(nslots, np.float32))
        s = 0
        for c, n in enumerate(SIZES):
            want = built.list_arrays(c)[name]
            assert np.array_equal(got[s:s + n].view(np.uint32), want.view(np.uint32)), (name, c)
            assert not got[s + n:s + (n + 31) // 32 * 32].view(np.uint32).any(), (name, c, "pad slots")
            s += (n + 31) // 32 * 32
    built.close(); idx.close()


# ---- 2. round trips --------------------------------------------------------------------------------------------------
ODD = np.array([0x80000000, 0x7FC00123, 0xFFA00001, 0x00000001, 0x807FFFFF, 0x7F800000, 0x3F800000], np.uint32)


@pytest.mark.parametrize("ex_bits,rot,dim", [(0, 1, 64), (2, 1, 100), (6, 0, 48), (6, 1, 960)])
def test_load_save_round_trip_of_odd_streams(ex_bits, rot, dim):
    """an independent-writer stream with random codes (pad lanes included), random ids and factors holding -0.0, NaN
    payloads and subnormals comes back byte for byte"""
    rng = np.random.default_rng(dim + ex_bits)
    D = (dim + 63) // 64 * 64 if rot == 1 else (dim + 15) // 16 * 16
    rot_bytes = rng.integers(0, 256, D // 2 if rot == 1 else D * D * 4, dtype=np.uint8).tobytes()
    exb = D * ex_bits // 8

    def f32(n, odd):
        v = rng.standard_normal(n).astype(np.float32).view(np.uint32)
        if odd and n:
            v[rng.integers(0, n, max(1, n // 3))] = ODD[rng.integers(0, ODD.size, max(1, n // 3))]
        return list(struct.unpack(f"<{n}f", v.tobytes()))

    clusters = []
    for n in SIZES:
        nb = (n + 31) // 32
        clusters.append({"centroid": f32(D, True), "ids": [int(x) for x in rng.integers(0, 1 << 63, n, dtype=np.uint64)],
                         "batch_data": rng.integers(0, 256, nb * (D * 4 + 384), dtype=np.uint8).tobytes(),
                         "ex_codes": [rng.integers(0, 256, exb, dtype=np.uint8).tobytes() for _ in range(n)],
                         "f_add_ex": f32(n, True) if ex_bits else [0.0] * n, "f_rescale_ex": f32(n, True) if ex_bits else [0.0] * n,
                         "delta": f32(n, True), "vl": f32(n, True)})
    stream = rbq1_writer.write_rbq1(dim, D, 0, rot, ex_bits, rot_bytes, clusters)
    idx = rq.IvfRabitqIndex.load_from_bytes(stream)
    _same(idx.save_to_bytes(), stream, "round trip")
    idx.close()


def test_reloaded_index_answers_identically(tmp_path):
    data, cent, assign = _dataset(960, 0, 17)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 5, True)
    a = rq.IvfRabitqIndex.from_built(built)
    p = tmp_path / "x.rbq"
    a.save_to_path(str(p))
    b = rq.IvfRabitqIndex.load_from_path(str(p))
    _same(p.read_bytes(), built.save_rbq1(), "save_to_path")
    q = make_dataset(64, 960, 4, 18)
    for k, nprobe in ((10, 4), (100, 8)):
        ra = a.batch_search_raw(q, rq.SearchParams(k, nprobe))
        rb = b.batch_search_raw(q, rq.SearchParams(k, nprobe))
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2])
        assert np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32))
    allowed = list(range(0, data.shape[0], 3))
    for qi in range(8):
        fa = a.search_filtered(q[qi], rq.SearchParams(10, 8), allowed)
        fb = b.search_filtered(q[qi], rq.SearchParams(10, 8), allowed)
        assert [(r.id, np.float32(r.score).tobytes()) for r in fa] == [(r.id, np.float32(r.score).tobytes()) for r in fb]
    built.close(); a.close(); b.close()


# ---- 3. streaming and errors -----------------------------------------------------------------------------------------
def _small_index(**kw):
    data, cent, assign = _dataset(kw.get("dim", 128), 0, 23)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 3, True)
    return built, data


@pytest.mark.parametrize("chunk", [4, 4100, 8192])
def test_forced_small_chunks_concatenate_to_the_stream(chunk):
    built, _ = _small_index()
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option("save_chunk", chunk)
    pieces = []

    class W:
        def write(self, b):
            pieces.append(bytes(b))
    idx.save_to_writer(W())
    want = built.save_rbq1()
    _same(b"".join(pieces), want, f"chunk {chunk}")
    assert len(pieces) > 3 and max(len(x) for x in pieces[1:-1]) <= chunk
    bio = io.BytesIO()
    idx.save_to_writer(bio)
    _same(bio.getvalue(), idx.save_to_bytes(), "BytesIO")
    built.close(); idx.close()


def test_failing_writer_gives_io_and_keeps_the_handle():
    built, data = _small_index()
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option("save_chunk", 4096)
    q = make_dataset(16, 128, 4, 29)
    before = idx.batch_search_raw(q, rq.SearchParams(10, 4))
    calls = []

    def cb(_u, _p, _n):
        calls.append(1)
        return 0 if len(calls) < 4 else 7
    rc = lib().rbq_index_save_rbq1_stream(idx._h, WRITE_FN(cb), None)
    assert rc == _abi.RBQ_IO and len(calls) == 4

    class Boom:
        def write(self, b):
            raise OSError("disk full")
    with pytest.raises(OSError, match="disk full"):
        idx.save_to_writer(Boom())
    after = idx.batch_search_raw(q, rq.SearchParams(10, 4))
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3]))
    _same(idx.save_to_bytes(), built.save_rbq1(), "after a failed save")
    built.close(); idx.close()


def test_multi_replica_handle_saves_the_same_bytes():
    built, _ = _small_index()
    idx = rq.IvfRabitqIndex.from_built(built, devices=[0, 0])
    assert lib().rbq_index_device_count(idx._h) == 2
    _same(idx.save_to_bytes(), built.save_rbq1(), "two replicas")
    built.close(); idx.close()


def test_save_beside_a_searching_thread():
    data, cent, assign = _dataset(960, 1, 41)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 1, 1, 5, True)
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option("save_chunk", 1 << 16)
    q = make_dataset(128, 960, 4, 42)
    base = idx.batch_search_raw(q, rq.SearchParams(10, 6))
    stop, bad, runs = threading.Event(), [], [0]

    def searcher():
        while not stop.is_set():
            r = idx.batch_search_raw(q, rq.SearchParams(10, 6))
            if not (np.array_equal(r[0], base[0]) and np.array_equal(r[1].view(np.uint32), base[1].view(np.uint32))):
                bad.append(1)
            runs[0] += 1
    t = threading.Thread(target=searcher)
    t.start()
    try:
        outs = [idx.save_to_bytes() for _ in range(3)]
    finally:
        stop.set()
        t.join()
    want = built.save_rbq1()
    for o in outs:
        _same(o, want, "concurrent save")
    assert not bad and runs[0] > 0
    built.close(); idx.close()


def test_refusals_have_messages():
    built, _ = _small_index()
    idx = rq.IvfRabitqIndex.from_built_without_recon(built)
    with pytest.raises(rq.RabitqError) as e:
        idx.save_to_bytes()
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "reconstruction factors" in str(e.value)
    with pytest.raises(rq.RabitqError) as e:
        idx.save_to_writer(io.BytesIO())
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    built.close(); idx.close()
    data, cent, assign = _dataset(64, 0, 3)
    mb = rq.builder.train_with_clusters(data, cent, assign, 7, 0, rq.RotatorType.NoRotation, 3, True)
    m = rq.IvfRabitqIndex.from_built(mb)
    with pytest.raises(rq.RabitqError) as e:
        m.save_to_bytes()
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "RBQ_ROTATOR_NONE" in str(e.value)
    mb.close(); m.close()


# ---- 4. GPU CRC ------------------------------------------------------------------------------------------------------
def test_gpu_crc32_matches_zlib():
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    big = torch.randint(0, 256, ((256 << 20) + 64,), dtype=torch.uint8, device="cuda", generator=g)
    host = big.cpu().numpy()
    base = big.data_ptr()
    for n in (0, 1, 3, 15, 16, 17, 255, 4095, 4096, 4097, 65537, (1 << 20) + 7, 4096 * 256 + 13, (250 << 20) + 5):
        for off in (0, 1, 3, 13):
            got = rq.IvfRabitqIndex.debug_crc32_device(base + off, n)
            assert got == zlib.crc32(host[off:off + n].tobytes()) & 0xFFFFFFFF, (n, off)
    for off in (0, 7):
        n = 256 << 20
        assert rq.IvfRabitqIndex.debug_crc32_device(base + off, n) == zlib.crc32(memoryview(host[off:off + n])) & 0xFFFFFFFF


# ---- 5. scale --------------------------------------------------------------------------------------------------------
def test_train_1m_save_load_search(tmp_path):
    import torch
    g = torch.Generator(device="cuda").manual_seed(11)
    n, dim = 1_000_000, 960
    means = torch.randn((256, dim), device="cuda", generator=g)
    x = means[torch.randint(0, 256, (n,), device="cuda", generator=g)] + 0.35 * torch.randn((n, dim), device="cuda", generator=g)
    idx = rq.IvfRabitqIndex.train(x, 4096, 7, 0, 1, 42, False)
    del x, means
    torch.cuda.empty_cache()
    p = tmp_path / "gist1m.rbq"
    idx.save_to_path(str(p))
    b = rq.IvfRabitqIndex.load_from_path(str(p))
    q = torch.randn((256, dim), generator=torch.Generator().manual_seed(3)).numpy()
    ra = idx.batch_search_raw(q, rq.SearchParams(10, 64))
    rb = b.batch_search_raw(q, rq.SearchParams(10, 64))
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2])
    assert np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32))
    _same(b.save_to_bytes(), p.read_bytes(), "1M reload -> save")
    idx.close(); b.close()
