"""BruteForceRabitqIndex.add / remove_ids / fetch_embeddings (rbq_bf_append, rbq_bf_remove_ids, rbq_bf_fetch_embeddings*,
include/rbq_bf_mutate.h) against the CPU builder.  A grown or shrunk index is, by contract, the index `train` gives over the rows it
then holds: the RBF1 stream of a mutated handle equals, byte for byte, the stream of the index uploaded from
builder.train_bruteforce over those rows (RBF1 holds every array of the index, so stream equality is array-for-array bit
equality).  Fetched rows are compared bit for bit with a NumPy restatement, written here, of the crate's IVF fetch_embedding against
the zero centroid over the CPU builder's arrays.  The reference is always the CPU builder, never the device path itself."""
import ctypes as C
import functools

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import bruteforce as bfm
from rabitq_rs_amd.index import _detail
import fetch_ref
from test_gpu_bf_train import first_difference, gaussian, special_rows

pytestmark = pytest.mark.gpu
BF = rq.BruteForceRabitqIndex
P = rq.BruteForceSearchParams
F32 = np.float32


def built_of(data, bits, metric, rotator, seed, faster):
    return rq.builder.train_bruteforce(data, bits, metric, rotator, seed, faster)


def cpu_bytes(data, bits, metric, rotator, seed, faster):
    built = built_of(data, bits, metric, rotator, seed, faster)
    idx = BF.from_built(built)
    try:
        return idx.save_to_bytes()
    finally:
        idx.close()
        built.close()


def cpu_index(data, bits, metric, rotator, seed, faster):
    """the CPU builder's index uploaded (the reference side of every comparison), with what add() needs to know"""
    built = built_of(data, bits, metric, rotator, seed, faster)
    try:
        return BF.from_built(built), dict(rescale="const" if faster else "optimal", t_const=built.t_const)
    finally:
        built.close()


def same(got, want, what=""):
    assert got == want, (what, first_difference(got, want))


# ---- append ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
@pytest.mark.parametrize("rotator,dim", [(1, 100), (1, 960), (0, 48)], ids=["fht-100", "fht-960", "matrix-48"])
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_append_matrix(bits, metric, rotator, dim, faster):
    """1003 old rows + 333 new: neither count nor their sum is a multiple of 32 or 64"""
    data = gaussian(1336, dim, 1000 * bits + 10 * dim + metric)
    seed = 7 + bits + dim
    idx, how = cpu_index(data[:1003], bits, metric, rotator, seed, faster)
    assert idx.add(data[1003:], **how) == 1003 and len(idx) == 1336
    same(idx.save_to_bytes(), cpu_bytes(data, bits, metric, rotator, seed, faster))
    idx.close()


@functools.lru_cache(maxsize=None)
def sizes_case(n_old, count):
    data = gaussian(n_old + count, 128, 100 * n_old + count)
    return data, cpu_bytes(data[:n_old], 7, 0, 1, 11, True), cpu_bytes(data, 7, 0, 1, 11, True)


@pytest.mark.parametrize("count", [1, 63, 65, 2000])
@pytest.mark.parametrize("n_old", [1, 31, 64, 257])
def test_append_sizes_chunks_and_input_kinds(n_old, count):
    import torch
    data, old_bytes, want = sizes_case(n_old, count)
    xd = torch.from_numpy(data[n_old:]).cuda()
    t = rq.builder.train_bruteforce(data[:1], 7, 0, 1, 11, True).t_const
    for chunk, new in ((0, data[n_old:]), (1, xd), (37, data[n_old:]), (37, xd)):
        idx = BF.load_from_bytes(old_bytes)  # (a loaded handle: rescale and t_const have to be given)
        with pytest.raises(rq.RabitqError, match="does not know what it was encoded with"):
            idx.add(new)
        assert idx.add(new, rescale="const", t_const=t, max_chunk_rows=chunk) == n_old
        same(idx.save_to_bytes(), want, (chunk, type(new).__name__))
        idx.close()


@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
@pytest.mark.parametrize("bits", [3, 7])
def test_append_to_a_loaded_handle(bits, faster):
    data = gaussian(900, 100, bits)
    idx, how = cpu_index(data[:613], bits, 1, 1, 3, faster)
    loaded = BF.load_from_bytes(idx.save_to_bytes())
    idx.close()
    loaded.add(data[613:], max_chunk_rows=1, **how)
    same(loaded.save_to_bytes(), cpu_bytes(data, bits, 1, 1, 3, faster))
    loaded.close()


def test_append_to_one_bit_handles_from_both_trainers():
    """a trained 1-bit index carries padded_dim/8 zero bytes of ex code per vector: the contract is on the saved bytes"""
    data = gaussian(700, 128, 2)
    want = cpu_bytes(data, 1, 0, 1, 2, True)
    a, how = cpu_index(data[:401], 1, 0, 1, 2, True)
    a.add(data[401:], **how)
    same(a.save_to_bytes(), want, "from_built")
    b = BF.train_on_device(data[:401], 1, 0, 1, 2, True)
    b.add(data[401:])  # (train_on_device remembers what it encoded with)
    same(b.save_to_bytes(), want, "train_on_device")
    c = BF.train(data[:401], 1, 0, 1, 2, False)
    c.add(data[401:])
    same(c.save_to_bytes(), cpu_bytes(data, 1, 0, 1, 2, False), "train")
    for i in (a, b, c):
        i.close()


def test_append_argument_errors_that_need_a_handle():
    data = gaussian(40, 64, 1)
    idx, how = cpu_index(data, 7, 0, 1, 5, True)
    lib, x = bfm.lib(), gaussian(3, 64, 2)
    before = idx.save_to_bytes()

    def call(vec, count, rescale, t):
        h = C.c_void_p(0xDEAD)
        rc = lib.rbq_bf_append(idx._h, vec, count, rescale, t, 0, C.byref(h))
        assert not h.value
        return rc, _detail()

    assert call(None, 3, 0, 1.5) == (rq._abi.RBQ_INVALID_CONFIG, "null vectors")
    assert call(x.ctypes.data, 0, 0, 1.5) == (rq._abi.RBQ_INVALID_CONFIG, "no vectors to append")
    assert call(x.ctypes.data, 1 << 32, 0, 1.5) == (rq._abi.RBQ_INVALID_CONFIG, "more than 2^32 vectors")
    rc, d = call(x.ctypes.data, 3, 7, 1.5)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and "unknown rescale mode" in d
    for t in (0.0, -1.0, float("nan")):
        rc, d = call(x.ctypes.data, 3, rq._abi.RESCALE_CONST, t)
        assert rc == rq._abi.RBQ_INVALID_CONFIG and "constant rescale factor" in d
    with pytest.raises(rq.RabitqError) as e:
        idx.add(gaussian(3, 48, 2), **how)
    assert e.value.kind == "DimensionMismatch"
    assert idx.save_to_bytes() == before and len(idx) == 40
    idx.close()


# ---- removal -----------------------------------------------------------------------------------------------------------------
N = 1003
SHAPES = {
    "first": lambda rng: [0],
    "last": lambda rng: [N - 1],
    "every-other": lambda rng: list(range(0, N, 2)),
    "run-over-32-64-256": lambda rng: list(range(29, 261)),
    "1%": lambda rng: rng.choice(N, 10, replace=False),
    "10%": lambda rng: rng.choice(N, 100, replace=False),
    "50%": lambda rng: rng.choice(N, 501, replace=False),
    "99%": lambda rng: rng.choice(N, 993, replace=False),
    "all-but-one": lambda rng: [i for i in range(N) if i != 517],
}
# Matrix dim 48: rows of 6 bytes (sign codes), 12 bytes (2-bit ex codes) and 36 bytes (6-bit): the gather's units of 2 and 4 bytes;
# FHT dim 100 (padded 128) and 960: sign rows of 16 and 120 bytes, 6-bit ex rows of 96 and 720 bytes: its units of 16 and 8 bytes
REMOVE_CONFIGS = [(0, 48, 1), (0, 48, 3), (0, 48, 7), (1, 100, 7), (1, 960, 7)]


@functools.lru_cache(maxsize=None)
def remove_case(rotator, dim, bits):
    data = gaussian(N, dim, 17 * dim + bits)
    return data, cpu_bytes(data, bits, 1, rotator, 9, True)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("rotator,dim,bits", REMOVE_CONFIGS, ids=["matrix-48-1bit", "matrix-48-3bit", "matrix-48-7bit", "fht-100", "fht-960"])
def test_remove_shapes(rotator, dim, bits, shape):
    data, _ = remove_case(rotator, dim, bits)
    gone = np.asarray(SHAPES[shape](np.random.default_rng(len(shape))), np.int64)
    keep = np.setdiff1d(np.arange(N), gone)
    idx, _ = cpu_index(data, bits, 1, rotator, 9, True)
    assert idx.remove_ids(gone) == gone.size and len(idx) == keep.size
    same(idx.save_to_bytes(), cpu_bytes(data[keep], bits, 1, rotator, 9, True))
    idx.close()


def test_remove_options():
    """unsorted ids with repeats and ids >= len; host ids and a CUDA tensor; out_removed; a set matching nothing; a set covering
    everything is refused and the old handle still searches"""
    import torch
    data, blob = remove_case(1, 100, 7)
    rng = np.random.default_rng(3)
    gone = rng.choice(N, 200, replace=False)
    ids = np.concatenate([gone.astype(np.uint64), gone[:50].astype(np.uint64), np.array([N, N + 5, 2 ** 40, 2 ** 64 - 1], np.uint64)])
    rng.shuffle(ids)
    want = cpu_bytes(data[np.setdiff1d(np.arange(N), gone)], 7, 1, 1, 9, True)
    for kind in ("host", "list", "cuda-i64", "cuda-u64"):
        idx = BF.load_from_bytes(blob)
        arg = {"host": ids, "list": [int(i) for i in ids], "cuda-i64": torch.from_numpy(ids.view(np.int64)).cuda(),
               "cuda-u64": torch.from_numpy(ids.view(np.int64)).cuda().view(torch.uint64)}[kind]
        assert idx.remove_ids(arg) == 200, kind
        same(idx.save_to_bytes(), want, kind)
        idx.close()
    idx = BF.load_from_bytes(blob)
    assert idx.remove_ids([N, N + 1, 2 ** 63]) == 0 and idx.save_to_bytes() == blob  # nothing matches: the result equals idx
    with pytest.raises(rq.RabitqError, match="the ids cover every vector of the index") as e:
        idx.remove_ids(np.arange(N + 3)[::-1])
    assert e.value.kind == "InvalidConfig"
    q = gaussian(4, 100, 1)
    ref = BF.load_from_bytes(blob)
    a, b = idx.batch_search_raw(q, P(10)), ref.batch_search_raw(q, P(10))
    assert idx.save_to_bytes() == blob and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    h = C.c_void_p(0xDEAD)
    for p, n, detail in ((None, 4, "null ids"), (ids.ctypes.data, 0, "no ids")):
        assert bfm.lib().rbq_bf_remove_ids(idx._h, p, n, None, C.byref(h)) == rq._abi.RBQ_INVALID_CONFIG and _detail() == detail and not h.value
    idx.close()
    ref.close()


# ---- special rows, sequences, the old handle, determinism -------------------------------------------------------------------
@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
@pytest.mark.parametrize("rotator,dim", [(1, 128), (0, 32)], ids=["fht-128", "matrix-32"])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_special_rows_through_add_and_remove(bits, rotator, dim, faster):
    """the zero vector, duplicates, denormals and the rows at the encoder's guards: appended, and removed around"""
    data = special_rows(dim, rotator, 77)
    idx, how = cpu_index(data[:2], bits, 0, rotator, 77, faster)
    idx.add(data[2:], **how)  # every special row goes through the appending encoder
    same(idx.save_to_bytes(), cpu_bytes(data, bits, 0, rotator, 77, faster), "add")
    gone = [2, 5, 12, 22, 32, 42, 52, 199]
    keep = np.setdiff1d(np.arange(200), gone)  # (the special rows stay and move)
    assert idx.remove_ids(gone) == len(gone)
    same(idx.save_to_bytes(), cpu_bytes(data[keep], bits, 0, rotator, 77, faster), "remove")
    idx.close()


@pytest.mark.parametrize("faster", [True, False], ids=["faster", "optimal"])
def test_sequence_equals_the_one_shot_build(faster):
    """add, add, remove, add, remove"""
    data = gaussian(900, 100, 13)
    held = list(range(300))
    idx = BF.train_on_device(data[:300], 7, 0, 1, 4, faster)
    assert idx.add(data[300:450]) == 300
    held += range(300, 450)
    assert idx.add(data[450:451]) == 450
    held += [450]
    gone = [0, 17, 299, 300, 449, 450]
    assert idx.remove_ids(gone) == 6
    held = [r for p, r in enumerate(held) if p not in gone]
    assert idx.add(data[451:900]) == len(held)
    held += range(451, 900)
    pos = np.random.default_rng(1).choice(len(held), 400, replace=False)
    assert idx.remove_ids(pos) == 400
    held = [r for p, r in enumerate(held) if p not in set(pos.tolist())]
    assert len(idx) == len(held)
    same(idx.save_to_bytes(), cpu_bytes(data[held], 7, 0, 1, 4, faster))
    idx.close()


def test_the_old_handle_is_only_read():
    lib = bfm.lib()
    data = gaussian(500, 100, 21)
    idx, how = cpu_index(data[:400], 3, 0, 1, 6, True)
    before = idx.save_to_bytes()
    x = np.ascontiguousarray(data[400:])
    h1, h2, removed = C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert lib.rbq_bf_append(idx._h, x.ctypes.data, 100, rq._abi.RESCALE_CONST, how["t_const"], 0, C.byref(h1)) == 0
    assert idx.save_to_bytes() == before and len(idx) == 400
    ids = np.arange(0, 400, 3, dtype=np.uint64)
    assert lib.rbq_bf_remove_ids(idx._h, ids.ctypes.data, ids.size, C.byref(removed), C.byref(h2)) == 0
    assert idx.save_to_bytes() == before and len(idx) == 400 and removed.value == ids.size
    grown, shrunk = BF(h1), BF(h2)
    same(grown.save_to_bytes(), cpu_bytes(data, 3, 0, 1, 6, True))
    same(shrunk.save_to_bytes(), cpu_bytes(data[:400][np.setdiff1d(np.arange(400), ids)], 3, 0, 1, 6, True))
    assert lib.rbq_bf_debug_append_carry_ns() > 0 and lib.rbq_bf_debug_remove_gather_ns() > 0
    for i in (idx, grown, shrunk):
        i.close()


def test_determinism():
    data = gaussian(3000, 256, 4)
    gone = np.random.default_rng(4).choice(2000, 700, replace=False)
    out = []
    for _ in range(2):
        idx = BF.train_on_device(data[:2000], 7, 0, 1, 4, False)
        idx.add(data[2000:])
        a = idx.save_to_bytes()
        idx.remove_ids(gone)
        out.append((a, idx.save_to_bytes()))
        idx.close()
    assert out[0] == out[1]


# ---- search on a mutated handle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
def test_a_mutated_handle_searches_like_the_cpu_built_index_of_the_same_rows(metric):
    data = gaussian(4300, 128, 31)
    data[2000:2400] = data[:400]  # equal distances: the heap's tie path
    gone = np.arange(100, 400)
    rows = np.setdiff1d(np.arange(4300), gone)  # (duplicates stay on both sides of the removed run)
    idx = BF.train_on_device(data[:3000], 7, metric, 1, 31, False)
    idx.add(data[3000:])
    idx.remove_ids(gone)
    built = built_of(data[rows], 7, metric, 1, 31, False)
    ref = BF.from_built(built)
    built.close()
    q = gaussian(32, 128, 32)
    for k in (10, 1000):
        a, b = ref.batch_search_raw(q, P(k)), idx.batch_search_raw(q, P(k))
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), k
    allowed = list(range(0, 4000, 7))
    assert ref.search_filtered(q[5], P(50), allowed) == idx.search_filtered(q[5], P(50), allowed)
    idx.close()
    ref.close()


# ---- fetch -------------------------------------------------------------------------------------------------------------------
def fetch_reference(built, ids):
    """fetch_embedding (src/ivf.rs:1247-1307) against the zero centroid over the CPU builder's arrays: code = ex + (bit << ex_bits);
    rotated = (0.0 + delta * code) + vl, every float op a float32 numpy op on its own and in the crate's order; then the rotator's
    inverse.  An id >= len: a zero row, found False."""
    a, h = built.arrays(), built.header
    D, ex_bits, n = int(h.padded_dim), int(h.ex_bits), len(built)
    ids = [int(i) for i in np.asarray(ids, np.uint64).reshape(-1)]
    out, found = np.zeros((len(ids), int(h.dim)), F32), np.zeros(len(ids), bool)
    hit = [k for k, i in enumerate(ids) if i < n]
    rows = np.zeros((len(hit), D), F32)
    for r, k in enumerate(hit):
        v = ids[k]
        bit = np.unpackbits(a["bin"][v], bitorder="big")[:D].astype(np.uint32)
        code = fetch_ref.ex_codes(a["ex"][v] if ex_bits else None, D, ex_bits) + (bit << np.uint32(ex_bits))
        t = a["delta"][v] * code.astype(F32)
        t = F32(0.0) + t
        rows[r] = t + a["vl"][v]
    if hit:
        out[hit] = fetch_ref.inverse_rotate(int(h.dim), D, int(h.rotator), built.rotator_blob(), rows)
        found[hit] = True
    return out, found


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


@pytest.mark.parametrize("rotator,dim", [(1, 128), (1, 100), (1, 960), (0, 32), (0, 48)],
                         ids=["fht-128", "fht-100", "fht-960", "matrix-32", "matrix-48"])
@pytest.mark.parametrize("bits", [1, 3, 7])
def test_fetch(bits, rotator, dim):
    """every id, repeats, ids >= len; the host entry and the device entry on a stream of its own"""
    import torch
    n = 301
    data = gaussian(n, dim, 50 * bits + dim)
    data[7] = 0.0  # (delta == 0: every rotated value is 0.0 + 0.0 * code + vl)
    built = built_of(data, bits, 0, rotator, 19, bits != 3)
    idx = BF.from_built(built)
    ids = np.array(list(range(n)) + [5, 5, 300, 0] + [n, n + 1, 2 ** 32, 2 ** 64 - 1] + [17], np.uint64)
    want, wfound = fetch_reference(built, ids)
    assert wfound.sum() == n + 5 and not want[~wfound].any()
    out, found = idx.fetch_embeddings(ids)
    assert np.array_equal(found, wfound) and bits_equal(out, want)
    d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    d_out = torch.full((ids.size, dim), float("nan"), dtype=torch.float32, device="cuda")
    d_found = torch.full((ids.size,), 9, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    idx.fetch_embeddings_device(d_ids.data_ptr(), ids.size, d_out.data_ptr(), d_found.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_found.cpu().numpy().astype(bool), wfound) and bits_equal(d_out.cpu().numpy(), want)
    one = idx.fetch_embedding(17)
    assert isinstance(one, list) and bits_equal(np.array(one, F32), want[17]) and idx.fetch_embedding(n) is None
    if bits == 7:  # a reconstruction of the rows, not of something else: 6-bit ex codes leave a few per cent of the norm
        assert np.linalg.norm(out[:n] - data) < 0.05 * np.linalg.norm(data)
    idx.close()
    built.close()


@pytest.mark.parametrize("rotator,dim", [(1, 100), (0, 48)], ids=["fht-100", "matrix-48"])
def test_fetch_after_add_and_after_remove_returns_the_renumbered_rows(rotator, dim):
    data = gaussian(500, dim, 5)
    idx, how = cpu_index(data[:300], 7, 1, rotator, 8, False)
    idx.add(data[300:], **how)
    ids = np.arange(502, dtype=np.uint64)
    built = built_of(data, 7, 1, rotator, 8, False)
    want, wfound = fetch_reference(built, ids)
    out, found = idx.fetch_embeddings(ids)
    assert np.array_equal(found, wfound) and bits_equal(out, want)
    built.close()
    gone = np.arange(10, 500, 4)
    keep = np.setdiff1d(np.arange(500), gone)
    idx.remove_ids(gone)
    built = built_of(data[keep], 7, 1, rotator, 8, False)
    want, wfound = fetch_reference(built, ids)
    out, found = idx.fetch_embeddings(ids)
    assert found.sum() == keep.size and np.array_equal(found, wfound) and bits_equal(out, want)
    idx.close()
    built.close()


def test_fetch_argument_errors():
    data = gaussian(20, 64, 1)
    idx, _ = cpu_index(data, 7, 0, 1, 5, True)
    lib = bfm.lib()
    ids, out, found = np.arange(4, dtype=np.uint64), np.zeros((4, 64), F32), np.zeros(4, np.uint8)
    assert lib.rbq_bf_fetch_embeddings(idx._h, None, 0, None, None) == 0  # n == 0: nothing to do
    assert lib.rbq_bf_fetch_embeddings(idx._h, None, 4, out.ctypes.data, found.ctypes.data) == rq._abi.RBQ_INVALID_CONFIG
    assert _detail() == "null ids / out / found"
    rc = lib.rbq_bf_fetch_embeddings_device(idx._h, ids.ctypes.data, 4, out.ctypes.data, found.ctypes.data, None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and "device memory" in _detail()  # host ids at the device entry
    idx.close()
