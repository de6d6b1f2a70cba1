"""fetch_embedding on the device (rbq_index_fetch_embeddings*, include/rbq.h; the crate's IvfRabitqIndex::fetch_embedding,
src/ivf.rs:1247-1307): every row bit for bit against the numpy restatement tests/fetch_ref.py over the index's own RBQ1 bytes,
for every creation path, metric, bit width and rotator; sparse / large / duplicated ids; errors; the device entry; chunking;
replicas; and searches running beside fetches."""
import threading

import numpy as np
import pytest

import fetch_ref
import rabitq_rs_amd as rq
import rbq1_writer
from conftest import make_dataset
from rabitq_rs_amd import _abi
from rabitq_rs_amd.index import lib

pytestmark = pytest.mark.gpu

# list sizes: empty lists, 1, 31, 32, 33 (one past a block) and larger ones
SIZES = [0, 1, 31, 32, 33, 300, 0, 65]


def _dataset(dim, metric, seed):
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    data = make_dataset(n, dim, 4, seed, normalize=(metric == 1))
    assign = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES)).astype(np.uint32)
    cent = np.stack([data[assign == c].mean(0) if s else data[c] for c, s in enumerate(SIZES)]).astype(np.float32)
    return data, cent, assign


def _bits_equal(got, want, what):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} values differ, first at {list(zip(*bad))[:3]}"


def _query_ids(stream, rng):
    """every id in stream order, a random subset with repeats, and ids that are not in the index"""
    ids = fetch_ref.all_ids(stream)
    present = set(ids.tolist())
    missing = [i for i in (int(ids.max()) + 1 if ids.size else 0, 1 << 40, (1 << 64) - 1, 7 << 33) if i not in present]
    sub = rng.choice(ids, size=min(200, 3 * ids.size), replace=True) if ids.size else np.zeros(0, np.uint64)
    return np.concatenate([ids, sub.astype(np.uint64), np.array(missing, np.uint64)])


def _check_index(idx, what, rng, stream=None):
    stream = idx.save_to_bytes() if stream is None else stream
    q = _query_ids(stream, rng)
    out, found = idx.fetch_embeddings(q)
    want, wfound = fetch_ref.fetch(stream, q)
    assert np.array_equal(found, wfound), what
    _bits_equal(out, want, what)
    assert not out[~found].view(np.uint32).any(), (what, "missing ids give zero rows")
    return q, out, found


def _stream_build(built, cent, data, assign, faster):
    sizes = np.bincount(assign, minlength=len(SIZES)).astype(np.uint32)
    sb = rq.StreamBuilder(built.hdr_ptr, cent, sizes, built.t_const if faster else None, rescale="const" if faster else "optimal")
    n = data.shape[0]
    for a, b in zip([0, 1, 200, n // 2], [1, 200, n // 2, n]):
        sb.push(data[a:b], assign[a:b], a)
    return sb.finish()


# ---- 1. every creation path, metric, bit width and rotator ---------------------------------------------------------------
@pytest.mark.parametrize("rot,dim", [(1, 64), (1, 100), (1, 960), (0, 64)], ids=["fhtkac-64", "fhtkac-100", "fhtkac-960", "matrix-64"])
@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_fetch_equals_reference(metric, bits, rot, dim):
    import torch
    rng = np.random.default_rng(dim + 10 * bits + metric)
    data, cent, assign = _dataset(dim, metric, 2000 + dim + 7 * bits + 3 * metric + rot)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    for faster in ((True, False) if bits > 1 else (True,)):
        built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rot, 91 + dim, faster)
        want_stream = rbq1_writer.from_built(built)
        paths = {
            "load_from_bytes": lambda: rq.IvfRabitqIndex.load_from_bytes(want_stream),
            "build_on_device": lambda: rq.IvfRabitqIndex.build_on_device(
                built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), data.shape[0], built.t_const if faster else None,
                rescale="const" if faster else "optimal"),
            "StreamBuilder": lambda: _stream_build(built, cent, data, assign, faster),
        }
        if faster:
            paths["from_built"] = lambda: rq.IvfRabitqIndex.from_built(built)
        for name, make in paths.items():
            idx = make()
            _check_index(idx, f"{name} faster={faster}", rng, want_stream if name in ("from_built", "load_from_bytes") else None)
            idx.close()
        built.close()


@pytest.mark.parametrize("bits,metric,rot,faster", [(7, 0, 1, False), (3, 1, 0, True)])
def test_fetch_after_train(bits, metric, rot, faster):
    data = make_dataset(3000, 128, 12, 71 + bits, normalize=(metric == 1))
    idx = rq.IvfRabitqIndex.train(data, 24, bits, metric, rot, 4243, faster)
    _check_index(idx, "train", np.random.default_rng(3))
    v = idx.fetch_embedding(5)
    assert v is not None and v.shape == (128,)
    assert idx.fetch_embedding(3000 + 10) is None
    idx.close()


def test_crate_sanity_properties_on_device():
    """src/tests.rs:1619-1735 on the device: 7 bits, every id within relative error 2.0, a missing id is None"""
    for rot, dim, n, nlist, seed in [(0, 64, 100, 4, 12345), (1, 128, 50, 8, 54321)]:
        data = np.random.default_rng(seed).random((n, dim), dtype=np.float32) * 2 - 1
        built = rq.builder.train(data, nlist, 7, 0, rot, seed, False, kmeans_iters=10)
        idx = rq.IvfRabitqIndex.from_built(built)
        for i in range(n):
            v = idx.fetch_embedding(i)
            assert v is not None and v.shape == (dim,)
            assert np.linalg.norm(v - data[i]) / max(np.linalg.norm(data[i]), 1e-7) < 2.0
        assert idx.fetch_embedding(n + 10) is None
        built.close(); idx.close()


# ---- 2. sparse, large and duplicated ids -------------------------------------------------------------------------------
@pytest.mark.parametrize("rot,dim,ex_bits", [(1, 100, 6), (1, 256, 2), (0, 48, 0)])
def test_sparse_large_duplicated_ids(rot, dim, ex_bits):
    """a stream with ids above 2^32, gaps, and ids repeated across and within clusters: the first (cluster, position)
    occurrence wins"""
    rng = np.random.default_rng(dim)
    data, cent, assign = _dataset(dim, 0, 17 + dim)
    built = rq.builder.train_with_clusters(data, cent, assign, ex_bits + 1, 0, rot, 5, True)
    h = built.header
    clusters = []
    pool = rng.integers(1 << 33, 1 << 62, 40, dtype=np.uint64)
    for c in range(int(h.n_lists)):
        a = built.list_arrays(c)
        n = len(a["ids"])
        ids = rng.integers(1 << 32, 1 << 63, n, dtype=np.uint64)
        k = n // 3
        if k:
            ids[rng.choice(n, k, replace=False)] = rng.choice(pool, k)  # shared across (and within) clusters
        clusters.append({"centroid": [float(v) for v in a["centroid"]], "ids": [int(i) for i in ids],
                         "batch_data": a["batch_data"].tobytes(),
                         "ex_codes": [a["ex_codes"][v].tobytes() if ex_bits else b"" for v in range(n)],
                         "f_add_ex": a["f_add_ex"].tolist(), "f_rescale_ex": a["f_rescale_ex"].tolist(),
                         "delta": a["delta"].tolist(), "vl": a["vl"].tolist()})
    stream = rbq1_writer.write_rbq1(int(h.dim), int(h.padded_dim), int(h.metric), int(h.rotator), ex_bits,
                                    built.rotator_blob(), clusters)
    idx = rq.IvfRabitqIndex.load_from_bytes(stream)
    q = np.concatenate([pool, _query_ids(stream, rng)])
    out, found = idx.fetch_embeddings(q)
    want, wfound = fetch_ref.fetch(stream, q)
    assert np.array_equal(found, wfound)
    _bits_equal(out, want, "sparse ids")
    built.close(); idx.close()


# ---- 3. errors and edge cases -------------------------------------------------------------------------------------------
def _small(rot=1, dim=64):
    data, cent, assign = _dataset(dim, 0, 3)
    return rq.builder.train_with_clusters(data, cent, assign, 7, 0, rot, 3, True), data


def test_errors_and_empty_calls():
    built, _ = _small()
    plain = rq.IvfRabitqIndex.from_built_without_recon(built)
    with pytest.raises(rq.RabitqError) as e:
        plain.fetch_embeddings([0, 1])
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "reconstruction factors" in str(e.value)
    plain.close()
    idx = rq.IvfRabitqIndex.from_built(built)
    L = lib()
    out = np.zeros((2, 64), np.float32)
    found = np.zeros(2, np.uint8)
    ids = np.array([0, 1], np.uint64)
    assert L.rbq_index_fetch_embeddings(idx._h, None, 2, out.ctypes.data, found.ctypes.data) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_index_fetch_embeddings(idx._h, ids.ctypes.data, 2, None, found.ctypes.data) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_index_fetch_embeddings(idx._h, ids.ctypes.data, 2, out.ctypes.data, None) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_index_fetch_embeddings(None, ids.ctypes.data, 2, out.ctypes.data, found.ctypes.data) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_index_fetch_embeddings(idx._h, None, 0, None, None) == _abi.RBQ_OK
    assert L.rbq_index_fetch_embeddings_device(idx._h, None, 0, None, None, None) == _abi.RBQ_OK
    assert L.rbq_index_fetch_embeddings_device(idx._h, None, 2, None, None, None) == _abi.RBQ_INVALID_CONFIG
    # host memory is not a device id array
    assert L.rbq_index_fetch_embeddings_device(idx._h, ids.ctypes.data, 2, out.ctypes.data, found.ctypes.data,
                                               None) == _abi.RBQ_INVALID_CONFIG
    o, f = idx.fetch_embeddings(np.zeros(0, np.uint64))
    assert o.shape == (0, 64) and f.shape == (0,)
    idx.close(); built.close()
    data, cent, assign = _dataset(64, 0, 3)
    nb = rq.builder.train_with_clusters(data, cent, assign, 7, 0, rq.RotatorType.NoRotation, 3, True)
    m = rq.IvfRabitqIndex.from_built(nb)
    with pytest.raises(rq.RabitqError) as e:
        m.fetch_embedding(0)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "RBQ_ROTATOR_NONE" in str(e.value)
    m.close(); nb.close()


def test_empty_index_finds_nothing():
    built, _ = _small()
    h = built.header
    empty = [{"centroid": [0.5] * int(h.padded_dim), "ids": [], "batch_data": b"", "ex_codes": [], "f_add_ex": [],
              "f_rescale_ex": [], "delta": [], "vl": []} for _ in range(3)]
    stream = rbq1_writer.write_rbq1(int(h.dim), int(h.padded_dim), 0, int(h.rotator), int(h.ex_bits), built.rotator_blob(), empty)
    idx = rq.IvfRabitqIndex.load_from_bytes(stream)
    assert len(idx) == 0
    out, found = idx.fetch_embeddings([0, 1, 1 << 50])
    assert not found.any() and not out.view(np.uint32).any()
    assert idx.fetch_embedding(0) is None
    idx.close(); built.close()


# ---- 4. numeric variant, device entry, chunking, replicas, concurrency --------------------------------------------------
def test_numeric_variant_does_not_change_fetch():
    built, data = _small(1, 960)
    idx = rq.IvfRabitqIndex.from_built(built)
    q = np.arange(len(data), dtype=np.uint64)
    base, _ = idx.fetch_embeddings(q)
    for v in ("native_avx2", "portable", "native_avx512"):
        idx.set_numeric_variant(v)
        out, _ = idx.fetch_embeddings(q)
        _bits_equal(out, base, v)
    idx.close(); built.close()


@pytest.mark.parametrize("rot,dim", [(1, 960), (0, 128)], ids=["fhtkac-960", "matrix-128"])
def test_device_entry_on_a_torch_stream(rot, dim):
    import torch
    built, data = _small(rot, dim)
    idx = rq.IvfRabitqIndex.from_built(built)
    rng = np.random.default_rng(dim)
    q = np.concatenate([rng.integers(0, len(data) + 50, 5000).astype(np.uint64), np.array([1 << 63], np.uint64)])
    want, wfound = idx.fetch_embeddings(q)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_ids = torch.from_numpy(q.view(np.int64)).cuda()
        d_out = torch.full((q.size, dim), 7.0, dtype=torch.float32, device="cuda")
        d_found = torch.full((q.size,), 9, dtype=torch.uint8, device="cuda")
    idx.fetch_embeddings_device(d_ids.data_ptr(), q.size, d_out.data_ptr(), d_found.data_ptr(), s.cuda_stream)
    s.synchronize()
    _bits_equal(d_out.cpu().numpy(), want, "device entry")
    assert np.array_equal(d_found.cpu().numpy().astype(bool), wfound)
    ref, _ = fetch_ref.fetch(idx.save_to_bytes(), q)
    _bits_equal(want, ref, "host entry")
    idx.close(); built.close()


@pytest.mark.parametrize("rot,dim,chunk", [(1, 100, 7), (1, 960, 64), (0, 64, 33)])
def test_host_chunks(rot, dim, chunk):
    built, data = _small(rot, dim)
    idx = rq.IvfRabitqIndex.from_built(built)
    q = np.random.default_rng(chunk).integers(0, len(data) + 20, 1000).astype(np.uint64)
    base, bfound = idx.fetch_embeddings(q)
    idx.set_option("fetch_chunk", chunk)
    out, found = idx.fetch_embeddings(q)
    _bits_equal(out, base, f"chunk {chunk}")
    assert np.array_equal(found, bfound)
    ref, rfound = fetch_ref.fetch(idx.save_to_bytes(), q)
    _bits_equal(out, ref, f"chunk {chunk} vs reference")
    assert np.array_equal(found, rfound)
    idx.close(); built.close()


def test_multi_replica_handle():
    built, data = _small(1, 128)
    idx = rq.IvfRabitqIndex.from_built(built, devices=[0, 0])
    assert idx.device_count() == 2
    q = np.arange(len(data) + 5, dtype=np.uint64)
    out, found = idx.fetch_embeddings(q)
    ref, rfound = fetch_ref.fetch(rbq1_writer.from_built(built), q)
    _bits_equal(out, ref, "two replicas")
    assert np.array_equal(found, rfound)
    idx.close(); built.close()


def test_search_beside_fetching_threads():
    data, cent, assign = _dataset(960, 1, 43)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 1, 1, 5, True)
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option("fetch_chunk", 100)
    qv = make_dataset(128, 960, 4, 44)
    base = idx.batch_search_raw(qv, rq.SearchParams(10, 6))
    ids = np.arange(len(data), dtype=np.uint64)
    want, _ = fetch_ref.fetch(rbq1_writer.from_built(built), ids)
    stop, bad, runs, fetch_bad = threading.Event(), [], [0], []

    def searcher():
        while not stop.is_set():
            r = idx.batch_search_raw(qv, rq.SearchParams(10, 6))
            if not (np.array_equal(r[0], base[0]) and np.array_equal(r[1].view(np.uint32), base[1].view(np.uint32))):
                bad.append(1)
            runs[0] += 1

    def fetcher():  # a second fetching thread: the first fetch of the handle builds the id map under its lock
        for _ in range(3):
            o, _ = idx.fetch_embeddings(ids)
            if not np.array_equal(o.view(np.uint32), want.view(np.uint32)):
                fetch_bad.append(1)
    t = threading.Thread(target=searcher)
    f = threading.Thread(target=fetcher)
    t.start(); f.start()
    try:
        outs = [idx.fetch_embeddings(ids)[0] for _ in range(3)]
    finally:
        f.join()
        stop.set()
        t.join()
    for o in outs:
        _bits_equal(o, want, "concurrent fetch")
    assert not bad and not fetch_bad and runs[0] > 0
    built.close(); idx.close()
