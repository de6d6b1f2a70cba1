"""`BruteForceRabitqIndex` (reference src/brute_force.rs) over the C ABI of include/rbq.h (rbq_bf_*).

Every vector is evaluated for every query on the GPU (k_bf_dist / k_bf_select); ids, counts and score bits equal the
crate's.  Training has two routes that give the same index, array for array and bit for bit: `train` runs the CPU builder
(builder.train_bruteforce) and uploads its arrays; `train_on_device` rotates, quantises and packs on the GPU
(rbq_bf_train_device) and writes the index in HBM directly, from a host array or a CUDA tensor."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi, _marshal
from .index import _check, _detail, lib  # noqa: F401  (shared error mapping; the rbq_bf_* entry points live in the same librbq.so)


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

    def __init__(self, handle, rescale=None):
        self._h = handle
        self._rescale = rescale  # (mode, t_const) the encoder ran with, where this object knows it: add()'s default

    @staticmethod
    def _dev(device):
        return -1 if device is None else int(device)

    @classmethod
    def train(cls, data, total_bits, metric, rotator_type, seed, use_faster_config, device=None):
        """`BruteForceRabitqIndex::train` (src/brute_force.rs:214-287) on the CPU builder, then uploaded."""
        from . import builder
        built = builder.train_bruteforce(data, total_bits, metric, rotator_type, seed, use_faster_config)
        idx = cls.from_built(built, device)
        idx._rescale = ("const", built.t_const) if use_faster_config else ("optimal", None)
        return idx

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
        torch = _marshal.torch_of(data)
        if torch is not None and data.is_cuda and device is not None and data.device.index != int(device):
            data = data.to(torch.device("cuda", int(device)))
        ptr, x = _marshal.rows_arg(data)  # (x owns what ptr names)
        if isinstance(x, np.ndarray):
            row0 = x[:1]
        else:
            row0, device = x[:1].cpu().numpy(), x.device.index
        small = builder.train_bruteforce(row0, total_bits, metric, rotator_type, seed, use_faster_config)  # (its own checks)
        try:
            h = C.c_void_p()
            _check(lib().rbq_bf_train_device(C.cast(small.hdr_ptr, C.c_void_p), ptr, int(shape[0]),
                                             _abi.RESCALE_CONST if use_faster_config else _abi.RESCALE_OPTIMAL, small.t_const,
                                             int(max_chunk_rows), cls._dev(device), C.byref(h)))
            return cls(h, ("const", small.t_const) if use_faster_config else ("optimal", None))
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
        return _marshal.owned_bytes(lambda p, n: _check(lib().rbq_bf_save_rbf1(self._h, p, n)), lib().rbq_bf_free_bytes)

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

    # -- growth, shrinking and read-back (include/rbq_bf_mutate.h) ----------------------------------------------------
    def add(self, data, rescale=None, t_const=None, max_chunk_rows=0):
        """FAISS-style add (rbq_bf_append): the rows of `data` [count][dim] (a host array or a CUDA tensor) join the index with the
        ids len(self) .. .  The index afterwards equals, array for array, `train` over the old and the new rows.  rescale
        ("const" / "optimal") and t_const default to what train or train_on_device encoded this object with; an object from
        load_from_* or from_built has to be given them.  The object's handle is swapped for the grown one and the old one
        closed.  Returns the id of the first new row."""
        from . import RabitqError
        from .index import _rescale
        rescale, t_const = _marshal.known_rescale(self._rescale, rescale, t_const)
        ptr, x = _marshal.rows_arg(data)  # (x owns what ptr names)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data must be [count][%d]" % self.dim)
        mode, t = _rescale(rescale, t_const)
        first = len(self)
        h = C.c_void_p()
        _check(lib().rbq_bf_append(self._h, ptr, int(x.shape[0]), mode, t, int(max_chunk_rows), C.byref(h)))
        self._rescale = (rescale, t_const)
        self._swap(h)
        return first

    def _swap(self, h):
        """The handle a mutation returned takes the place of the old one, which is closed."""
        old, self._h = self._h, h
        lib().rbq_bf_destroy(old)

    def remove_ids(self, ids):
        """FAISS IndexFlat-style remove_ids (rbq_bf_remove_ids): the vectors at the positions `ids` (a host array, a list, or a
        CUDA int64 / uint64 tensor; any order, repeats allowed, ids >= len ignored) leave the index.  A brute-force index has no id
        array: the id of a vector is its position, so the survivors keep their order and are RENUMBERED 0 .. len - 1.  The index
        afterwards equals, array for array, `train` over the rows that stay.  The object's handle is swapped for the shrunk one
        and the old one closed; the remembered rescale mode stays.  Returns the number of rows removed; an empty `ids` returns 0
        without a call."""
        n, p, _ids = _marshal.ids_arg(ids)  # (_ids owns what p names)
        if n == 0:
            return 0
        h, removed = C.c_void_p(), C.c_uint64()
        _check(lib().rbq_bf_remove_ids(self._h, p, n, C.byref(removed), C.byref(h)))
        self._swap(h)
        return int(removed.value)

    def fetch_embeddings(self, ids):
        """rbq_bf_fetch_embeddings: (out [n, dim] f32, found [n] bool).  Row i is the crate's IVF fetch_embedding of vector ids[i]
        against the zero centroid, bit for bit; an id >= len gives a zero row and found False."""
        return _marshal.fetch_embeddings(lib().rbq_bf_fetch_embeddings, self._h, self.dim, ids)

    def fetch_embedding(self, vector_id):
        """The reconstructed vector [dim] as a list of floats, or None when the id is not in the index."""
        out, found = self.fetch_embeddings([vector_id])
        return out[0].tolist() if found[0] else None

    def fetch_embeddings_device(self, d_ids, n, d_out, d_found, stream=None):
        """rbq_bf_fetch_embeddings_device: n u64 ids at d_ids (device memory of the index's device) -> d_out [n][dim] f32,
        d_found [n] u8, enqueued on `stream` (a hipStream_t as int, None = default stream)."""
        _marshal.fetch_embeddings_device(lib().rbq_bf_fetch_embeddings_device, self._h, d_ids, n, d_out, d_found, stream)

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
