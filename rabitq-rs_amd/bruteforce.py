"""`BruteForceRabitqIndex` (reference src/brute_force.rs) over the C ABI of include/rbq.h (rbq_bf_*).

Every vector is evaluated for every query on the GPU (k_bf_dist / k_bf_select); ids, counts and score bits equal the
crate's.  Training has two routes that give the same index, array for array and bit for bit: `train` runs the CPU builder
(builder.train_bruteforce) and uploads its arrays; `train_on_device` rotates, quantises and packs on the GPU
(rbq_bf_train_device) and writes the index in HBM directly, from a host array or a CUDA tensor."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from .index import _check, _detail  # noqa: F401  (shared error mapping)

_BOUND = False


def lib():
    """librbq.so with the rbq_bf_* signatures bound (the same library object as index.lib())."""
    global _BOUND
    from .index import lib as base
    L = base()
    if not _BOUND:
        vp = C.c_void_p
        L.rbq_bf_create.restype = C.c_int
        L.rbq_bf_create.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
        L.rbq_bf_train_device.restype = C.c_int
        L.rbq_bf_train_device.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_float, C.c_uint64, C.c_int, C.POINTER(vp)]
        L.rbq_bf_load_rbf1.restype = C.c_int
        L.rbq_bf_load_rbf1.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp)]
        L.rbq_bf_save_rbf1.restype = C.c_int
        L.rbq_bf_save_rbf1.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
        L.rbq_bf_free_bytes.restype = None
        L.rbq_bf_free_bytes.argtypes = [C.POINTER(C.c_uint8)]
        L.rbq_bf_destroy.restype = None
        L.rbq_bf_destroy.argtypes = [vp]
        L.rbq_bf_len.restype = C.c_uint64
        L.rbq_bf_len.argtypes = [vp]
        for n in ("rbq_bf_dim", "rbq_bf_padded_dim"):
            getattr(L, n).restype = C.c_uint32
            getattr(L, n).argtypes = [vp]
        L.rbq_bf_search_batch.restype = C.c_int
        L.rbq_bf_search_batch.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, vp, vp]
        L.rbq_bf_debug_heap_stats.restype = None
        L.rbq_bf_debug_heap_stats.argtypes = [vp, vp]
        L.rbq_bf_debug_set_chunk_vectors.restype = C.c_uint64
        L.rbq_bf_debug_set_chunk_vectors.argtypes = [C.c_uint64]
        L.rbq_bf_debug_select_launches.restype = C.c_uint64
        L.rbq_bf_debug_select_launches.argtypes = []
        _BOUND = True
    return L


@dataclass(frozen=True)
class BruteForceSearchParams:
    top_k: int


@dataclass(frozen=True)
class BruteForceSearchResult:
    id: int
    score: float


def _filter_words(allowed_ids):
    allowed = np.asarray(sorted(set(int(i) for i in allowed_ids)), dtype=np.uint64)
    nbits = int(allowed.max()) + 1 if allowed.size else 0
    words = np.zeros((nbits + 31) // 32 or 1, np.uint32)
    if allowed.size:
        np.bitwise_or.at(words, (allowed >> np.uint64(5)).astype(np.int64),
                         (np.uint32(1) << (allowed & np.uint64(31)).astype(np.uint32)))
    return words, nbits


class BruteForceRabitqIndex:
    """Device-resident brute-force RaBitQ index; methods mirror reference src/brute_force.rs."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _dev(device):
        return -1 if device is None else int(device)

    @classmethod
    def train(cls, data, total_bits, metric, rotator_type, seed, use_faster_config, device=None):
        """`BruteForceRabitqIndex::train` (src/brute_force.rs:214-287) on the CPU builder, then uploaded."""
        from . import builder
        return cls.from_built(builder.train_bruteforce(data, total_bits, metric, rotator_type, seed, use_faster_config), device)

    @classmethod
    def train_on_device(cls, data, total_bits, metric, rotator_type, seed, use_faster_config, device=None, max_chunk_rows=0):
        """`BruteForceRabitqIndex::train` (src/brute_force.rs:214-285) with the rotation and quantisation on the GPU
        (rbq_bf_train_device).  `data` [n][dim] is a host array or a CUDA tensor.  The crate's checks and messages come first, in
        its order.  The header — rotator, and t_const for the faster configuration — depends only on (dim, bits, rotator, seed):
        it is taken from the CPU builder over a single row.  `max_chunk_rows` bounds the rows encoded per pass (0: sized from the
        encoder's scratch budget); the index does not depend on it and equals `train`'s."""
        from . import RabitqError, builder
        shape = tuple(getattr(data, "shape", None) or np.shape(data))
        if len(shape) != 2 or shape[0] == 0:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "training data must be non-empty")
        if not 1 <= int(total_bits) <= 16:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "total_bits must be between 1 and 16")
        is_tensor = type(data).__module__.startswith("torch")
        if is_tensor:
            import torch
            if data.is_cuda:
                if device is not None and data.device.index != int(device):
                    data = data.to(torch.device("cuda", int(device)))
                x = data.to(dtype=torch.float32).contiguous()
                ptr, row0, device = x.data_ptr(), x[:1].cpu().numpy(), x.device.index
            else:
                data, is_tensor = data.numpy(), False
        if not is_tensor:
            x = np.ascontiguousarray(data, dtype=np.float32)
            ptr, row0 = x.ctypes.data, x[:1]
        small = builder.train_bruteforce(row0, total_bits, metric, rotator_type, seed, use_faster_config)  # (its own checks)
        try:
            h = C.c_void_p()
            _check(lib().rbq_bf_train_device(C.cast(small.hdr_ptr, C.c_void_p), ptr, int(shape[0]),
                                             _abi.RESCALE_CONST if use_faster_config else _abi.RESCALE_OPTIMAL, small.t_const,
                                             int(max_chunk_rows), cls._dev(device), C.byref(h)))
            return cls(h)
        finally:
            small.close()

    @classmethod
    def from_built(cls, built, device=None):
        h = C.c_void_p()
        _check(lib().rbq_bf_create(C.cast(built.hdr_ptr, C.c_void_p), C.cast(built.view_ptr, C.c_void_p), cls._dev(device), C.byref(h)))
        return cls(h)

    @classmethod
    def load_from_bytes(cls, data, device=None):
        """`load_from_reader` (src/brute_force.rs:395-520) straight into HBM."""
        h = C.c_void_p()
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        _check(lib().rbq_bf_load_rbf1(buf, len(data), cls._dev(device), C.byref(h)))
        return cls(h)

    @classmethod
    def load_from_path(cls, path, device=None):
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            from . import RabitqError
            raise RabitqError(_abi.RBQ_IO, str(e))
        return cls.load_from_bytes(data, device)

    def save_to_bytes(self):
        """`save_to_writer` (src/brute_force.rs:305-386), byte for byte."""
        p = C.POINTER(C.c_uint8)()
        n = C.c_uint64()
        _check(lib().rbq_bf_save_rbf1(self._h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            lib().rbq_bf_free_bytes(p)

    def save_to_path(self, path):
        data = self.save_to_bytes()
        try:
            with open(path, "wb") as f:
                f.write(data)
        except OSError as e:
            from . import RabitqError
            raise RabitqError(_abi.RBQ_IO, str(e))

    def __len__(self):
        return lib().rbq_bf_len(self._h)

    def is_empty(self):
        return len(self) == 0

    @property
    def dim(self):
        return lib().rbq_bf_dim(self._h)

    @property
    def padded_dim(self):
        return lib().rbq_bf_padded_dim(self._h)

    def batch_search_raw(self, queries, params, filter_words=None, filter_nbits=0):
        """Returns (ids[nq,k] u64, scores[nq,k] f32, counts[nq] u32)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, qd = q.shape
        k = int(params.top_k)
        ids = np.full((nq, k), np.iinfo(np.uint64).max, np.uint64)
        scores = np.full((nq, k), np.nan, np.float32)
        counts = np.zeros(nq, np.uint32)
        fw = np.ascontiguousarray(filter_words, dtype=np.uint32) if filter_words is not None else None
        _check(lib().rbq_bf_search_batch(self._h, q.ctypes.data, nq, qd, k, fw.ctypes.data if fw is not None else None,
                                         int(filter_nbits), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    @staticmethod
    def _results(ids, scores, counts, q):
        return [BruteForceSearchResult(int(ids[q, i]), float(scores[q, i])) for i in range(int(counts[q]))]

    def search(self, query, params):
        """`search` (src/brute_force.rs:525-531)."""
        ids, scores, counts = self.batch_search_raw(np.asarray(query, np.float32)[None, :], params)
        return self._results(ids, scores, counts, 0)

    def search_filtered(self, query, params, allowed_ids):
        """`search_filtered` (src/brute_force.rs:535-543); `allowed_ids` plays the RoaringBitmap."""
        words, nbits = _filter_words(allowed_ids)
        ids, scores, counts = self.batch_search_raw(np.asarray(query, np.float32)[None, :], params, words, nbits)
        return self._results(ids, scores, counts, 0)

    def batch_search(self, queries, params):
        """`search` for every row of `queries`, results in input order."""
        ids, scores, counts = self.batch_search_raw(queries, params)
        return [self._results(ids, scores, counts, q) for q in range(ids.shape[0])]

    def heap_stats(self):
        """{pushes, tie_pushes} of the BinaryHeap emulation since the index was created (rbq_bf_debug_heap_stats)."""
        out = np.zeros(2, np.uint64)
        lib().rbq_bf_debug_heap_stats(self._h, out.ctypes.data)
        return {"pushes": int(out[0]), "tie_pushes": int(out[1])}

    def close(self):
        if self._h:
            lib().rbq_bf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
