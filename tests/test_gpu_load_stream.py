"""rbq_index_load_rbq1_stream (include/rbq_persist.h): an RBQ1 stream loaded span by span, checksummed, checked and laid out
by the GPU, against the whole-buffer loader rbq_index_load_rbq1 — every device array bit for bit, at every span size, and
the same (code, detail) for every corrupted or truncated stream of tests/load_stream_cases.py.  Every comparison is exact."""
import ctypes as C
import io
import re

import numpy as np
import pytest

import load_stream_cases as cases
import rabitq_rs_amd as rq
from conftest import make_dataset
from rabitq_rs_amd import _abi
from rabitq_rs_amd.index import READ_FN, _detail, lib

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 31, 32, 33, 300, 0, 65]  # (tests/test_gpu_save.py) empty lists, 1, one short of a block, one past it, 10 blocks
ARRAYS = ("blocks", "ids", "ex", "fadd_ex", "fres_ex", "bsum", "lsum", "bsumx", "centroids", "list_gb0", "list_n", "cent_hi",
          "cent_lo", "cnorm2", "delta", "vl")
DEFAULT_SPAN = 64 << 20


def _stream(dim, metric, ex_bits, rot):
    rng = np.random.default_rng(900 + dim + 7 * ex_bits + 3 * metric + rot)
    data = make_dataset(sum(SIZES), dim, 4, 100 + dim + ex_bits, normalize=(metric == 1))
    assign = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES)).astype(np.uint32)
    cent = np.stack([data[assign == c].mean(0) if s else data[c] for c, s in enumerate(SIZES)]).astype(np.float32)
    built = rq.builder.train_with_clusters(data, cent, assign, ex_bits + 1, metric, rot, 77 + dim, True)
    out = bytes(built.save_rbq1())
    built.close()
    return out


def _arrays(idx):
    """every array rbq_debug_copy_index can name, as bytes (the library says how long each is)"""
    out = {}
    for name in ARRAYS:
        rc = lib().rbq_debug_copy_index(idx._h, name.encode(), C.byref(C.c_uint8()), 0)
        n = 0 if rc == 0 else int(re.search(r"have (\d+) bytes", _detail()).group(1))
        buf = np.empty(n, np.uint8)
        if n:
            idx.debug_copy_index(name, buf)
        out[name] = buf.tobytes()
    return out


class Reader:
    """a recording rbq_read_fn over bytes; fail_at = k: the k-th call (1-based) returns non-zero"""

    def __init__(self, data, fail_at=0):
        self.buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        self.total, self.calls, self.fail_at = len(data), [], fail_at
        self.fn = READ_FN(self._cb)

    def _cb(self, _user, off, dst, n):
        self.calls.append((off, n))
        if len(self.calls) == self.fail_at:
            return 5
        if off + n > self.total:
            return 9
        C.memmove(dst, C.addressof(self.buf) + off, n)
        return 0


def stream_load(data, devices=None, fail_at=0):
    """(rc, detail, index or None, reader)"""
    r = Reader(data, fail_at)
    h = C.c_void_p()
    n, dev = rq.IvfRabitqIndex._devices(None, devices)
    rc = lib().rbq_index_load_rbq1_stream(r.fn, None, len(data), n, dev, C.byref(h))
    detail = _detail() if rc else ""
    assert (rc == 0) == bool(h.value), (rc, h.value)
    return rc, detail, (rq.IvfRabitqIndex(h) if h.value else None), r


def whole_load(data, devices=None):
    h = C.c_void_p()
    n, dev = rq.IvfRabitqIndex._devices(None, devices)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    rc = lib().rbq_index_load_rbq1(buf, len(data), n, dev, C.byref(h))
    detail = _detail() if rc else ""
    assert (rc == 0) == bool(h.value), (rc, h.value)
    return rc, detail, (rq.IvfRabitqIndex(h) if h.value else None)


class span:
    """rbq_debug_set_load_span for a with block; the default comes back in every case"""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def __enter__(self):
        lib().rbq_debug_set_load_span(self.nbytes)

    def __exit__(self, *exc):
        lib().rbq_debug_set_load_span(0)


_REF = {}


def _reference(dim, metric, ex_bits, rot):
    """the stream, the whole-buffer loader's arrays and its answers to 16 queries; computed once per shape"""
    key = (dim, metric, ex_bits, rot)
    if key not in _REF:
        s = _stream(dim, metric, ex_bits, rot)
        idx = rq.IvfRabitqIndex.load_from_bytes(s)
        q = make_dataset(16, dim, 4, 5 + dim, normalize=(metric == 1))
        _REF[key] = (s, _arrays(idx), q, idx.batch_search_raw(q, rq.SearchParams(10, 4))[:3])
        idx.close()
    return _REF[key]


def _assert_same_index(idx, ref, what):
    s, arrays, q, res = ref
    got = _arrays(idx)
    for name in ARRAYS:
        assert len(got[name]) == len(arrays[name]), (what, name, len(got[name]), len(arrays[name]))
        if got[name] != arrays[name]:
            a, b = np.frombuffer(got[name], np.uint8), np.frombuffer(arrays[name], np.uint8)
            raise AssertionError(f"{what}: {name} differs at bytes {np.nonzero(a != b)[0][:8]} of {a.size}")
    assert idx.save_to_bytes() == s, (what, "save_to_bytes")
    ids, scores, counts = idx.batch_search_raw(q, rq.SearchParams(10, 4))[:3]
    assert np.array_equal(ids, res[0]) and np.array_equal(counts, res[2]), (what, "search ids / counts")
    assert np.array_equal(scores.view(np.uint32), res[1].view(np.uint32)), (what, "search score bits")


SHAPES = [(1, 64), (1, 100), (1, 960), (1, 2048), (0, 64)]
SHAPE_IDS = ["fhtkac-64", "fhtkac-100", "fhtkac-960", "fhtkac-2048", "matrix-64"]


# ---- 1. array parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot,dim", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ex_bits", [0, 2, 6])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_streamed_load_equals_whole_buffer_load(metric, ex_bits, rot, dim):
    ref = _reference(dim, metric, ex_bits, rot)
    rc, detail, idx, _ = stream_load(ref[0])
    assert rc == 0, detail
    assert len(idx) == sum(SIZES) and idx.cluster_count() == len(SIZES)
    _assert_same_index(idx, ref, "default span")
    idx.close()


# ---- 2. span independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot,dim,ex_bits,metric", [(1, 2048, 6, 0), (1, 100, 2, 1), (1, 64, 0, 0), (0, 64, 6, 1), (1, 960, 6, 1)],
                         ids=["fhtkac-2048-7bit", "fhtkac-100-3bit", "fhtkac-64-1bit", "matrix-64-7bit", "fhtkac-960-7bit"])
def test_result_does_not_depend_on_the_span(rot, dim, ex_bits, metric):
    ref = _reference(dim, metric, ex_bits, rot)
    D = (dim + 63) // 64 * 64 if rot == 1 else dim
    unit = D * 4 + 384  # the largest indivisible unit: one batch record (8576 bytes at 2048)
    n_calls = {}
    for nbytes in (1, 3 * unit + 52, 0):  # the minimum (1 is raised to one unit), an odd size of a few units, the default
        with span(nbytes):
            rc, detail, idx, r = stream_load(ref[0])
        assert rc == 0, (nbytes, detail)
        _assert_same_index(idx, ref, f"span {nbytes}")
        idx.close()
        limit = max(nbytes, unit) if nbytes else DEFAULT_SPAN
        assert all(0 <= off and n >= 1 and off + n <= len(ref[0]) and n <= limit for off, n in r.calls), (nbytes, limit)
        n_calls[nbytes] = len(r.calls)
    # the minimum span cuts inside every section of the 300-vector list: far more reads than the default's single span
    assert n_calls[1] > n_calls[3 * unit + 52] > n_calls[0]
    assert lib().rbq_debug_set_load_span(0) == 0  # (the default was restored)


def test_set_load_span_returns_the_previous_value():
    try:
        assert lib().rbq_debug_set_load_span(4096) == 0
        assert lib().rbq_debug_set_load_span(12345) == 4096
        assert lib().rbq_debug_set_load_span(0) == 12345
    finally:
        lib().rbq_debug_set_load_span(0)


# ---- 3. callback discipline ---------------------------------------------------------------------------------------------
def test_reads_stay_inside_the_stream_and_junk_behind_the_crc_is_ignored():
    ref = _reference(960, 0, 6, 1)
    s = ref[0]
    junk = s + bytes(np.random.default_rng(1).integers(0, 256, 1000, dtype=np.uint8))
    for nbytes in (1, 0):
        with span(nbytes):
            rc, detail, idx, r = stream_load(junk)
        assert rc == 0, detail
        _assert_same_index(idx, ref, f"junk behind the CRC, span {nbytes}")
        idx.close()
        limit = max(nbytes, 960 * 4 + 384) if nbytes else DEFAULT_SPAN
        assert all(off + n <= len(junk) and 1 <= n <= limit for off, n in r.calls)
        assert max(off + n for off, n in r.calls) == len(s)  # nothing behind the stored CRC was asked for


def test_null_arguments_are_invalid_config():
    s = cases.base_stream()
    r = Reader(s)
    h = C.c_void_p()
    assert lib().rbq_index_load_rbq1_stream(r.fn, None, len(s), 1, None, None) == _abi.RBQ_INVALID_CONFIG
    assert lib().rbq_index_load_rbq1_stream(READ_FN(0), None, len(s), 1, None, C.byref(h)) == _abi.RBQ_INVALID_CONFIG
    assert not h.value and not r.calls


# ---- 4. error parity ----------------------------------------------------------------------------------------------------
def _parity(named, spans):
    bad = []
    for name, data in named:
        want = whole_load(data)
        if want[2] is not None:
            want[2].close()
        for nbytes in spans:
            with span(nbytes):
                got = stream_load(data)
            if got[2] is not None:
                got[2].close()
            if got[:2] != want[:2]:
                bad.append((name, nbytes, got[:2], want[:2]))
    return bad


def test_header_and_field_errors_equal_the_whole_buffer_loader():
    s = cases.base_stream()
    named = cases.header_cases(s)
    assert not _parity(named, (1, 2333, 0))
    # (the corpus does what it says: the good stream loads, the others do not, with more than one message)
    answers = {n: whole_load(d) for n, d in named}
    for n, a in answers.items():
        if a[2] is not None:
            a[2].close()
    assert answers["good"][0] == 0 and answers["junk after the CRC"][0] == 0
    assert sum(1 for a in answers.values() if a[0] == 0) == 2
    assert "Unsupported ex_bits" in answers["ex_bits 4, consistent stream"][1]
    assert answers["no clusters"] == (_abi.RBQ_INVALID_CONFIG, "nlist must be positive", None)
    assert len({a[1] for a in answers.values()}) >= 17


def test_truncated_streams_equal_the_whole_buffer_loader():
    s = cases.base_stream()
    named = cases.truncation_cases(s)
    assert len(named) > 150
    assert not _parity(named, (1, 2333))
    assert all(whole_load(d)[:2] == (_abi.RBQ_IO, "failed to fill whole buffer") for _, d in named[::7])


def test_the_first_error_in_file_order_wins():
    s = cases.base_stream()
    named = cases.order_cases(s)
    assert not _parity(named, (1, 2333, 0))
    answers = {n: whole_load(d)[1] for n, d in named}
    assert answers["prefix in list 1 + batch_data length in list 2"].startswith("ex_code_packed length mismatch")
    assert answers["prefix + batch_data length, both in list 1"].startswith("batch_data length mismatch")
    assert answers["prefix in list 1 + bit flip in list 3"].startswith("ex_code_packed length mismatch")
    # a good stream still loads and searches after all of that
    ref = _reference(64, 0, 6, 1)
    rc, detail, idx, _ = stream_load(ref[0])
    assert rc == 0, detail
    _assert_same_index(idx, ref, "after the corpus")
    idx.close()


def test_invalid_device_comes_after_the_stream_errors():
    s = cases.base_stream()
    for data in (s, cases._flip(s, 100), s[:500]):
        want = whole_load(data, devices=[99])
        with span(1):
            got = stream_load(data, devices=[99])
        assert got[:3] == want[:3] and got[2] is None


# ---- 5. failing reader --------------------------------------------------------------------------------------------------
def test_a_failing_reader_is_io_at_every_call():
    s = cases.base_stream()
    with span(1):
        rc, detail, idx, good = stream_load(s)
        assert rc == 0, detail
        idx.close()
        n = len(good.calls)
        assert n > 20  # header, rotator, two fields per list, a dozen spans, the stored CRC
        for k in range(1, n + 1):
            rc, detail, idx, r = stream_load(s, fail_at=k)
            assert (rc, detail, idx) == (_abi.RBQ_IO, "read callback failed", None), k
            assert len(r.calls) == k  # the load stops at the failing call
    ref = _reference(64, 0, 6, 1)
    rc, detail, idx, _ = stream_load(ref[0])
    assert rc == 0, detail
    _assert_same_index(idx, ref, "after the failing readers")
    idx.close()


# ---- 6. Python ----------------------------------------------------------------------------------------------------------
def test_load_from_reader_on_file_objects(tmp_path):
    ref = _reference(960, 0, 6, 1)
    s = ref[0]
    idx = rq.IvfRabitqIndex.load_from_reader(io.BytesIO(s))
    _assert_same_index(idx, ref, "BytesIO")
    idx.close()
    p = tmp_path / "x.rbq"
    p.write_bytes(s)
    with open(p, "rb") as f, span(100000):
        idx = rq.IvfRabitqIndex.load_from_reader(f)
    _assert_same_index(idx, ref, "file")
    idx.close()
    p2 = tmp_path / "y.bin"
    p2.write_bytes(b"thirteen byte" + s)
    with open(p2, "rb") as f:
        f.seek(13)
        idx = rq.IvfRabitqIndex.load_from_reader(f)
    _assert_same_index(idx, ref, "file at offset 13")
    idx.close()

    class ReadOnly:  # no readinto
        def __init__(self, data):
            self._f = io.BytesIO(data)
            self.seek, self.tell, self.read = self._f.seek, self._f.tell, self._f.read
    idx = rq.IvfRabitqIndex.load_from_reader(ReadOnly(s))
    _assert_same_index(idx, ref, "read() only")
    idx.close()
    with pytest.raises(rq.RabitqError) as e:
        rq.IvfRabitqIndex.load_from_reader(io.BytesIO(s[:-5]))
    assert e.value.code == _abi.RBQ_IO and "failed to fill whole buffer" in str(e.value)


def test_an_exception_in_the_file_object_comes_back():
    s = _reference(960, 0, 6, 1)[0]

    class Boom(io.BytesIO):
        calls = 0

        def readinto(self, b):
            Boom.calls += 1
            if Boom.calls == 6:
                raise OSError("medium removed")
            return super().readinto(b)
    with span(1), pytest.raises(OSError, match="medium removed"):
        rq.IvfRabitqIndex.load_from_reader(Boom(s))
    assert Boom.calls == 6
    idx = rq.IvfRabitqIndex.load_from_reader(io.BytesIO(s))  # and the next load is fine
    assert len(idx) == sum(SIZES)
    idx.close()


# ---- 7. two devices -----------------------------------------------------------------------------------------------------
def test_streamed_load_onto_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    ref = _reference(960, 0, 6, 1)
    rc, detail, a = whole_load(ref[0], devices=[0, 1])
    assert rc == 0, detail
    rc, detail, b, _ = stream_load(ref[0], devices=[0, 1])
    assert rc == 0, detail
    assert a.device_count() == b.device_count() == 2
    for rep in (0, 1):
        a.set_option("debug_replica", rep)
        b.set_option("debug_replica", rep)
        assert _arrays(a) == _arrays(b), rep
    a.close(); b.close()
