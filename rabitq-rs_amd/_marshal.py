"""Argument marshalling shared by index.py, bruteforce.py, mstg.py and builder.py: Python values to the pointers the C ABI takes,
and back.  Each helper has one job; what a call means (its checks, their order, what happens to the handle) stays with the caller.

A helper that returns a raw pointer returns the object that owns the memory with it.  The caller keeps that object in a local
until the C call has returned: the pointer is only as alive as the object is."""
import ctypes as C
import sys

import numpy as np

from . import _abi


def torch_of(x):
    """The torch module when `x` is a torch tensor, else None.  torch is never imported for it: a tensor cannot exist before
    torch is loaded, so host inputs work in a Python without torch."""
    torch = sys.modules.get("torch")
    return torch if torch is not None and isinstance(x, torch.Tensor) else None


def ids_arg(ids):
    """(n, pointer, keep-alive) of [n] u64 ids: a list, any iterable, a NumPy array or a CPU tensor (converted on the host), or a
    CUDA int64 / uint64 tensor (used in place)."""
    torch = torch_of(ids)
    if torch is not None and ids.is_cuda:
        if ids.dtype not in (torch.int64, torch.uint64):
            from . import RabitqError
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "ids on the device must be int64 or uint64")
        v = ids.contiguous().reshape(-1)
        return int(v.numel()), C.c_void_p(v.data_ptr()), v
    if torch is not None:
        ids = ids.numpy()
    if not isinstance(ids, np.ndarray):  # (numpy would make float64 of a list that mixes ints below and above 2^63)
        ids = np.asarray(ids if hasattr(ids, "__len__") else list(ids), dtype=np.uint64)
    v = np.ascontiguousarray(ids).astype(np.uint64).reshape(-1)
    return int(v.size), C.c_void_p(v.ctypes.data), v


def rows_arg(data):
    """(pointer, keep-alive) of [rows][dim] f32: a CUDA tensor is used in place when it is contiguous f32 (converted on its
    device otherwise); anything else becomes a contiguous host array.  The keep-alive has .ndim and .shape either way."""
    torch = torch_of(data)
    if torch is not None:
        t = data.to(dtype=torch.float32).contiguous()
        if t.is_cuda:
            return C.c_void_p(t.data_ptr()), t
        data = t.numpy()
    h = np.ascontiguousarray(data, dtype=np.float32)
    return C.c_void_p(h.ctypes.data), h


def query_arg(queries, dtype=None):
    """(keep-alive, RBQ_RAW_* code) of a query argument (option "query_dtype"): a contiguous NumPy array or torch tensor whose
    elements the library reads as they are, and what they are.  numpy.float32 -> f32 as ever; numpy.float16 -> f16; torch.half ->
    f16 and torch.bfloat16 -> bf16, on the host or on a device; a numpy.uint16 array holds bit patterns and needs `dtype` "f16" or
    "bf16" (set_rerank_vectors' convention).  Anything else becomes f32 on the host (a tensor: where it lives), as before.
    `dtype` "f16" with other host data converts with astype(numpy.float16), "f32" widens: the caller's rounding, never the library's.
    data_ptr(keep-alive) is the pointer."""
    from . import RabitqError
    code = None
    if dtype is not None:
        if isinstance(dtype, str) and dtype not in _abi.RAW_DTYPES:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "unknown query dtype %r (one of %s)" % (dtype, ", ".join(_abi.RAW_DTYPES)))
        code = _abi.RAW_DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    torch = torch_of(queries)
    if torch is not None:
        own = {torch.float16: _abi.RAW_F16, torch.bfloat16: _abi.RAW_BF16}.get(queries.dtype, _abi.RAW_F32)
        if code is None:
            code = own
        if code != own or queries.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            want = {_abi.RAW_F32: torch.float32, _abi.RAW_F16: torch.float16, _abi.RAW_BF16: torch.bfloat16}.get(code)
            if want is None:
                raise RabitqError(_abi.RBQ_INVALID_CONFIG, "unknown query dtype %r" % (dtype,))
            queries = queries.to(dtype=want)
        return queries.contiguous(), code
    if isinstance(queries, np.ndarray) and queries.dtype == np.uint16:
        if code not in (_abi.RAW_F16, _abi.RAW_BF16):
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, 'uint16 queries are bit patterns: pass dtype="f16" or dtype="bf16"')
        return np.ascontiguousarray(queries), code
    if code is None:
        code = _abi.RAW_F16 if isinstance(queries, np.ndarray) and queries.dtype == np.float16 else _abi.RAW_F32
    if code == _abi.RAW_BF16:
        raise RabitqError(_abi.RBQ_INVALID_CONFIG, "bf16 queries on the host are a uint16 array of bit patterns or a torch.bfloat16 tensor")
    if code not in (_abi.RAW_F32, _abi.RAW_F16):
        raise RabitqError(_abi.RBQ_INVALID_CONFIG, "unknown query dtype %r" % (dtype,))
    return np.ascontiguousarray(queries, dtype=np.float16 if code == _abi.RAW_F16 else np.float32), code


def data_ptr(x):
    """The address of the first element of what query_arg returned."""
    return int(x.data_ptr()) if torch_of(x) is not None else int(x.ctypes.data)


def on_device(x):
    return torch_of(x) is not None and x.is_cuda


def known_rescale(remembered, rescale, t_const):
    """(rescale, t_const) of an add(): what the caller passed, else what the object remembers it was encoded with."""
    if rescale is None:
        if remembered is None:
            from . import RabitqError
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "this index does not know what it was encoded with (a loaded index does not "
                              "store it): pass rescale= and t_const= to add()")
        rescale, t_known = remembered
        if t_const is None:
            t_const = t_known
    return rescale, t_const


def owned_bytes(call, free):
    """The bytes of a buffer the library allocates: call(byref(uint8_t*), byref(uint64_t)) fills the pair (and raises on failure),
    free(pointer) releases it after the copy."""
    p, n = C.POINTER(C.c_uint8)(), C.c_uint64()
    call(C.byref(p), C.byref(n))
    try:
        return C.string_at(p, n.value)
    finally:
        free(p)


def writer_callback(fileobj):
    """(rbq_write_fn, errors): every chunk goes to fileobj.write; an exception it raises is parked in `errors` and stops the
    save (the callback returns 1).  The caller re-raises errors[0] after the C call."""
    err = []

    def cb(_user, p, n):
        try:
            fileobj.write(C.string_at(p, n) if n else b"")
            return 0
        except BaseException as e:  # noqa: BLE001 - handed back to the caller after the C call returns
            err.append(e)
            return 1
    return _abi.WRITE_FN(cb), err


def reader_callback(fileobj, start):
    """(rbq_read_fn, errors): the range (offset, len) of the stream is read from fileobj at start + offset, straight into the
    destination with readinto where the object has it, else through read.  A short read returns 1; an exception is parked as in
    writer_callback."""
    readinto = getattr(fileobj, "readinto", None)
    err = []

    def cb(_user, off, dst, n):
        try:
            fileobj.seek(start + off)
            view = memoryview((C.c_ubyte * n).from_address(dst)).cast("B")
            got = 0
            while got < n:
                if readinto is not None:
                    k = readinto(view[got:])
                else:
                    chunk = fileobj.read(n - got)
                    k = len(chunk)
                    view[got:got + k] = chunk
                if not k:
                    return 1  # the object ended before the range did
                got += k
            return 0
        except BaseException as e:  # noqa: BLE001
            err.append(e)
            return 1
    return _abi.READ_FN(cb), err


def fetch_embeddings(fn, handle, dim, ids):
    """rbq_*_fetch_embeddings: (out [n, dim] f32, found [n] bool) of the host ids."""
    from .index import _check
    q = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
    n = int(q.size)
    out = np.empty((n, dim), np.float32)
    found = np.empty(n, np.uint8)
    _check(fn(handle, q.ctypes.data, n, out.ctypes.data, found.ctypes.data))
    return out, found.astype(bool)


def fetch_embeddings_device(fn, handle, d_ids, n, d_out, d_found, stream):
    """rbq_*_fetch_embeddings_device on device pointers given as ints; `stream` a hipStream_t as int, None = default stream."""
    from .index import _check
    _check(fn(handle, C.c_void_p(d_ids), int(n), C.c_void_p(d_out), C.c_void_p(d_found), C.c_void_p(stream) if stream else None))
