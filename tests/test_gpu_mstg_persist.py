"""`.mstg` persistence on the GPU (include/rbq_mstg_persist.h): the device-assembled stream equals the independent writer's
(tests/mstg_file.py over the CPU builder's arrays) byte for byte whatever the chunk size, a loaded index equals the saved one
array for array and answer for answer, writer-made files survive load -> save unchanged, and every malformed file is refused
with the loader's code (malformed inputs that are validated before use).  Shapes: tests/mstg_persist_cases.py."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import mstg_file as mf
import mstg_persist_cases as pc
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, index, mstg

pytestmark = pytest.mark.gpu

COMBOS = [(16, 1, 0, True), (16, 3, 1, True), (16, 7, 0, False), (48, 3, 0, False), (48, 7, 1, True), (64, 1, 1, False),
          (64, 7, 0, True)]
ARRAYS = ("list_gb0", "list_n", "centroids", "blocks", "ids", "bsum", "lsum", "bsumx", "delta", "vl", "rnorm", "cent_hi", "cent_lo",
          "cnorm2", "ex", "fadd_ex", "fres_ex")


def _build(case):
    return rq.build_postings_on_device(case.x, case.c, case.bits, case.metric, closure_epsilon=pc.EPS, max_replicas=pc.REPLICAS,
                                       faster_config=case.faster)


def _arrays(idx, D, ex, nlist=8):
    Dc = (D + 63) // 64 * 64
    ln = idx.debug_copy_index("list_n", np.empty(nlist, np.uint32))
    nb = int(((ln + 31) // 32).sum())
    cpu_u = 128 // ex if ex else 1
    w4 = ((D // 16 + cpu_u - 1) // cpu_u) if ex else 0
    sizes = {"list_gb0": nlist * 4, "list_n": nlist * 4, "centroids": nlist * D * 4, "blocks": nb * (Dc * 4 + 384), "ids": nb * 256,
             "bsum": nb * 32, "lsum": nlist * 32, "bsumx": nb * 32, "delta": nb * 128, "vl": nb * 128, "rnorm": nb * 128,
             "cent_hi": nlist * D * 2, "cent_lo": nlist * D * 2, "cnorm2": nlist * 4}
    if ex:
        sizes.update({"ex": nb * 32 * w4 * 256, "fadd_ex": nb * 128, "fres_ex": nb * 128})
    assert set(sizes) <= set(ARRAYS)
    return {name: idx.debug_copy_index(name, np.empty(nbytes, np.uint8)) for name, nbytes in sizes.items()}


def _same_arrays(a, b):
    assert a.keys() == b.keys()
    for name in a:
        bad = np.nonzero(a[name] != b[name])[0]
        assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at {bad[:5]}"


def _queries(case, nq=64):
    rng = np.random.default_rng(11)
    return (case.x[rng.integers(0, len(case.x), nq)] + 0.05 * rng.standard_normal((nq, case.D))).astype(np.float32)


def _answers(h, q):
    host = mstg.mstg_search(h, q, 10, 6, 0.6, return_lists=True)
    dev = mstg.mstg_search(h, torch.from_numpy(q).cuda(), 10, 6, 0.6, return_lists=True)
    torch.cuda.synchronize()
    return [np.ascontiguousarray(a).view(np.uint8) for a in host] + [a.cpu().numpy().view(np.uint8) for a in dev]


@pytest.fixture(scope="module")
def case3():
    return pc.Case(D=16, bits=3, metric=0, faster=True)


@pytest.mark.parametrize("D,bits,metric,faster", COMBOS)
def test_save_equals_the_independent_writer_for_every_chunk_size_and_loads_back(D, bits, metric, faster):
    case = pc.Case(D, bits, metric, faster)
    dev = _build(case)
    got = mstg.save_mstg_bytes(dev, case.cfg)
    assert len(got) == len(case.bytes)
    bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(case.bytes, np.uint8))[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    for chunk in (64, 119, 4096):  # below one record, one record of D = 16 at 7 bits (odd), several records
        dev.set_option("mstg_chunk", chunk)
        out = io.BytesIO()
        mstg.save_mstg(dev, case.cfg, out)
        assert out.getvalue() == got, chunk
    dev.set_option("mstg_chunk", 0)
    # load(save(x)) == x: every array, every answer
    back, cfg = mstg.load_mstg(got)
    assert {k: cfg[k] for k in ("rabitq_bits", "metric", "faster_config", "max_posting_size", "default_ef_search")} == \
        {k: case.cfg[k] for k in ("rabitq_bits", "metric", "faster_config", "max_posting_size", "default_ef_search")}
    assert len(back) == len(dev) == len(case.pair_vec) and back.cluster_count() == 8
    _same_arrays(_arrays(dev, D, bits - 1), _arrays(back, D, bits - 1))
    q = _queries(case)
    a, b = _answers(dev, q), _answers(back, q)
    assert int(a[2].view(np.uint32).sum()) > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert mstg.save_mstg_bytes(back, cfg) == got
    assert mstg.memory_usage(back) == mstg.memory_usage(dev) > 0
    back.close()
    dev.close()


def test_writer_made_files_survive_load_and_save(case3, monkeypatch, tmp_path):
    """the 3-bit file's empty list carries RabitqConfig::default() (7, None); the second file holds NaN, -0.0 and denormal bit
    patterns in every factor that the format keeps"""
    files = [case3.bytes]
    lists = [dict(L) for L in case3.lists]
    odd = np.array([0x7FC00001, 0x80000000, 0xFFC12345, 0x00000001, 0x7F800000], np.uint32).view(np.float32)
    for L in lists:
        n = len(L["ids"])
        for j, f in enumerate(mf.FACTORS):
            a = np.array(L[f], np.float32)
            a[:] = np.resize(np.roll(odd, j), n)
            L[f] = a
    files.append(mf.write(case3.cfg, lists, case3.t_const))
    _, parsed, _, _, _ = mf.parse(files[0])
    assert parsed[7]["config"] == (7, None) and parsed[1]["config"][0] == 3
    for i, b in enumerate(files):
        h, cfg = mstg.load_mstg(b)
        assert mstg.save_mstg_bytes(h, cfg) == b
        h.close()
        # the stream loader over a file, with spans of single headers and blocks
        p = tmp_path / f"f{i}.mstg"
        p.write_bytes(b)
        monkeypatch.setenv("RBQ_MSTG_LOAD_SPAN", "64")
        h, cfg = mstg.load_mstg(str(p))
        monkeypatch.delenv("RBQ_MSTG_LOAD_SPAN")
        out = io.BytesIO()
        mstg.save_mstg(h, cfg, out)
        assert out.getvalue() == b
        h.close()


def test_every_corruption_is_refused_and_a_good_load_follows(case3):
    for name, bad, piece in pc.corruptions(case3):
        with pytest.raises(rq.RabitqError) as e:
            mstg.load_mstg(bad)
        assert e.value.code == _abi.RBQ_INVALID_PERSISTENCE and e.value.detail and piece in e.value.detail, (name, e.value.detail)
        assert rq.builder.mstg_file_check(bad)[1] == e.value.detail, name  # the CPU check states the same refusal
    tiny = pc.tiny_file()
    for cut in pc.truncations(tiny, 37) + [tiny[:-1], tiny[:-4]]:
        with pytest.raises(rq.RabitqError) as e:
            mstg.load_mstg(cut)
        assert e.value.code == _abi.RBQ_INVALID_PERSISTENCE
    _, L, _, _, _ = mf.parse(tiny)
    bad = bytearray(tiny)
    bad[L[0]["rec0"] + 109 - 3] = 1  # f_rescale_ex of a 1-bit record
    with pytest.raises(rq.RabitqError) as e:
        mstg.load_mstg(pc.fix_crc(bad))
    assert e.value.code == _abi.RBQ_INVALID_PERSISTENCE and "1-bit" in e.value.detail
    h, cfg = mstg.load_mstg(case3.bytes)
    assert len(h) == len(case3.pair_vec)
    ids, _, cnt = mstg.mstg_search(h, _queries(case3, 4), 5, 6, 0.6)
    assert (cnt > 0).all()
    h.close()
    h, _ = mstg.load_mstg(tiny)
    assert len(h) == 3
    h.close()


def test_a_failing_writer_is_io_and_refused_handles_are_invalid_config(case3):
    dev = _build(case3)
    cfg = _abi.MstgConfig.from_dict(case3.cfg)
    for fail_at in (0, 1, 3):
        calls = []

        def cb(_user, _p, n, fail_at=fail_at):
            calls.append(n)
            return 7 if len(calls) > fail_at else 0
        dev.set_option("mstg_chunk", 4096)
        rc = index.lib().rbq_mstg_save_stream(dev._h, C.byref(cfg), index.WRITE_FN(cb), None)
        assert rc == _abi.RBQ_IO and len(calls) == fail_at + 1
    dev.set_option("mstg_chunk", 0)
    assert mstg.save_mstg_bytes(dev, case3.cfg) == case3.bytes
    assert (mstg.mstg_search(dev, _queries(case3, 4), 5, 6, 0.6)[2] > 0).all()
    for wrong, piece in ((dict(case3.cfg, rabitq_bits=7), "rabitq_bits"), (dict(case3.cfg, metric=1), "metric"),
                         (dict(case3.cfg, centroid_precision=4), "centroid_precision")):
        with pytest.raises(rq.RabitqError) as e:
            mstg.save_mstg_bytes(dev, wrong)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG and piece in e.value.detail
    dev.close()
    # the same lists through rbq_index_create_with_recon: a posting-list handle without residual norms
    ref = rq.IvfRabitqIndex.from_built(case3.built)
    with pytest.raises(rq.RabitqError) as e:
        mstg.save_mstg_bytes(ref, case3.cfg)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "residual norms" in e.value.detail
    ref.close()
    built = rq.builder.train(case3.x, 4, 3, 0, rq.RotatorType.FhtKacRotator, 42, True, kmeans_iters=2)
    ivf = rq.IvfRabitqIndex.from_built(built)
    with pytest.raises(rq.RabitqError) as e:
        mstg.save_mstg_bytes(ivf, case3.cfg)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "not an MSTG handle" in e.value.detail
    ivf.close()
    built.close()


@pytest.mark.parametrize("metric,bits,faster", [("euclidean", 7, True), ("angular", 3, False)])
def test_mstgindex_fit_save_load_batch_query(tmp_path, metric, bits, faster):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((600, 32)).astype(np.float32)
    a = rq.MstgIndex(32, metric, max_posting_size=40, branching_factor=4, rabitq_bits=bits, faster_config=faster, hnsw_m=16,
                     hnsw_ef_construction=123, centroid_precision="fp16", default_ef_search=9, pruning_epsilon=0.5,
                     closure_epsilon=0.25, max_replicas=3, balance_weight=0.75).fit(x)  # (floats exact in f32: the file stores f32)
    base = tmp_path / "idx"
    a.save(base)
    assert (tmp_path / "idx.mstg").exists() and sorted(p.name for p in tmp_path.iterdir()) == ["idx.mstg"]
    b = rq.MstgIndex.load(base)
    assert repr(a) == repr(b) and len(a) == len(b) == 600
    assert a.config() == b.config() and b.centroid_precision == "fp16" and b.hnsw_ef_construction == 123
    assert np.array_equal(a.centroids, b.centroids)
    assert a.get_memory_usage() == b.get_memory_usage() > 0
    q = x[:50] + 0.01
    ra, rb = a.batch_query(q, 7), b.batch_query(q, 7)
    assert sum(len(r) for r in ra) > 0
    for u, v in zip(ra, rb):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    parsed_cfg = mf.parse((tmp_path / "idx.mstg").read_bytes())[0]
    assert parsed_cfg["hnsw_m"] == 16 and parsed_cfg["centroid_precision"] == 2 and parsed_cfg["faster_config"] == faster
    with pytest.raises(rq.RabitqError) as e:
        rq.MstgIndex.load(tmp_path / "missing")
    assert e.value.code == _abi.RBQ_IO
