"""rabitq-rs_amd/_marshal.py without a GPU and without a library: what ids_arg, rows_arg and known_rescale hand to a C call, that
every pointer is the data pointer of the object returned with it, and what the two stream callbacks do with a file object that
raises, ends early or has no readinto.  (The CUDA-tensor branches run in the GPU tests of add, remove_ids and the MSTG calls.)"""
import ctypes as C
import io

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, _marshal

try:
    import torch
except ImportError:
    torch = None


def u64_at(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(n,)).copy() if n else np.zeros(0, np.uint64)


@pytest.mark.parametrize("ids,want", [
    ([1, 2 ** 63 + 5], [1, 2 ** 63 + 5]),                          # numpy alone would make float64 of it and lose the low bits
    ((i * i for i in range(5)), [0, 1, 4, 9, 16]),                # a generator has no len()
    (np.array([7, 3, 7], np.int64), [7, 3, 7]),
    (np.arange(10, dtype=np.uint64)[::3], [0, 3, 6, 9]),          # a non-contiguous view
    (np.arange(6, dtype=np.uint32).reshape(2, 3), [0, 1, 2, 3, 4, 5]),
], ids=["mixed-above-2^63", "generator", "int64", "strided", "2d-u32"])
def test_ids_arg_host_inputs(ids, want):
    n, p, keep = _marshal.ids_arg(ids)
    assert n == len(want) and isinstance(p, C.c_void_p)
    assert isinstance(keep, np.ndarray) and keep.dtype == np.uint64 and keep.flags.c_contiguous and keep.ndim == 1
    assert p.value == keep.ctypes.data  # the pointer is the kept object's own
    assert u64_at(p, n).tolist() == want == keep.tolist()


def test_ids_arg_empty_list():
    n, p, keep = _marshal.ids_arg([])
    assert n == 0 and keep.size == 0 and keep.dtype == np.uint64


@pytest.mark.skipif(torch is None, reason="torch is not installed")
def test_ids_arg_cpu_tensor():
    t = torch.tensor([5, 2 ** 40, 9], dtype=torch.int64)
    n, p, keep = _marshal.ids_arg(t)
    assert n == 3 and isinstance(keep, np.ndarray) and p.value == keep.ctypes.data and keep.tolist() == [5, 2 ** 40, 9]
    assert _marshal.torch_of(t) is torch and _marshal.torch_of(keep) is None and _marshal.torch_of([1]) is None


def f32_at(p, shape):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=shape).copy()


@pytest.mark.parametrize("kind", ["float64", "fortran", "cpu_tensor"])
def test_rows_arg_host_inputs(kind):
    base = (np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5)
    if kind == "float64":
        data = base
    elif kind == "fortran":
        data = np.asfortranarray(base.astype(np.float32))
        assert not data.flags.c_contiguous
    else:
        if torch is None:
            pytest.skip("torch is not installed")
        data = torch.from_numpy(base).t().contiguous().t()  # a float64 tensor whose rows are not contiguous
        assert not data.is_contiguous()
    p, keep = _marshal.rows_arg(data)
    assert isinstance(p, C.c_void_p) and isinstance(keep, np.ndarray)
    assert keep.dtype == np.float32 and keep.flags.c_contiguous and keep.shape == (3, 4) and keep.ndim == 2
    assert p.value == keep.ctypes.data  # the pointer is the kept object's own
    assert np.array_equal(f32_at(p, (3, 4)), base.astype(np.float32))


def test_rows_arg_uses_a_contiguous_f32_array_in_place():
    x = np.ones((2, 8), np.float32)
    p, keep = _marshal.rows_arg(x)
    assert keep is x and p.value == x.ctypes.data


def test_known_rescale():
    assert _marshal.known_rescale(None, "optimal", None) == ("optimal", None)          # given: nothing needs remembering
    assert _marshal.known_rescale(("const", 1.5), "optimal", 2.0) == ("optimal", 2.0)  # given wins over remembered
    assert _marshal.known_rescale(("const", 1.5), None, None) == ("const", 1.5)        # remembered, both
    assert _marshal.known_rescale(("const", 1.5), None, 2.5) == ("const", 2.5)         # remembered mode, the caller's t_const
    with pytest.raises(rq.RabitqError) as e:
        _marshal.known_rescale(None, None, 1.0)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    assert e.value.detail == ("this index does not know what it was encoded with (a loaded index does not store it): "
                              "pass rescale= and t_const= to add()")


class Boom(Exception):
    pass


def test_writer_callback():
    sink = io.BytesIO()
    fn, err = _marshal.writer_callback(sink)
    assert isinstance(fn, _abi.WRITE_FN)
    buf = C.create_string_buffer(b"abcdef", 6)
    assert fn(None, C.addressof(buf), 6) == 0 and fn(None, None, 0) == 0 and fn(None, C.addressof(buf) + 2, 3) == 0
    assert sink.getvalue() == b"abcdefcde" and err == []

    class Full:
        def write(self, b):
            raise Boom("disk full")
    fn, err = _marshal.writer_callback(Full())
    assert fn(None, C.addressof(buf), 6) == 1 and len(err) == 1 and isinstance(err[0], Boom)


class OnlyRead:
    """a file object without readinto that hands out at most 3 bytes per read"""

    def __init__(self, data):
        self._f = io.BytesIO(data)

    def seek(self, *a):
        return self._f.seek(*a)

    def read(self, n):
        return self._f.read(min(n, 3))


@pytest.mark.parametrize("make", [io.BytesIO, OnlyRead], ids=["readinto", "read-only"])
def test_reader_callback(make):
    data = bytes(range(40))
    fn, err = _marshal.reader_callback(make(data), 8)  # the stream starts at byte 8 of the object
    assert isinstance(fn, _abi.READ_FN)
    dst = (C.c_ubyte * 16)()
    assert fn(None, 4, C.addressof(dst), 10) == 0
    assert bytes(dst[:10]) == data[12:22] and bytes(dst[10:]) == bytes(6) and err == []
    assert fn(None, 20, C.addressof(dst), 16) == 1 and err == []  # 12 bytes are left: a short read is an error, not an exception
    assert fn(None, 0, C.addressof(dst), 16) == 0 and bytes(dst) == data[8:24]


def test_reader_callback_parks_the_exception():
    class Broken(io.BytesIO):
        def readinto(self, b):
            raise Boom("bad sector")
    fn, err = _marshal.reader_callback(Broken(bytes(32)), 0)
    dst = (C.c_ubyte * 8)()
    assert fn(None, 0, C.addressof(dst), 8) == 1 and len(err) == 1 and isinstance(err[0], Boom)


def test_owned_bytes_copies_then_frees():
    src = (C.c_uint8 * 5)(1, 2, 3, 4, 5)
    freed = []

    def call(p, n):
        C.cast(p, C.POINTER(C.POINTER(C.c_uint8)))[0] = C.cast(src, C.POINTER(C.c_uint8))
        C.cast(n, C.POINTER(C.c_uint64))[0] = 5
    assert _marshal.owned_bytes(call, lambda p: freed.append(C.addressof(p.contents))) == bytes([1, 2, 3, 4, 5])
    assert freed == [C.addressof(src)]
