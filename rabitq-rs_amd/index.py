"""`IvfRabitqIndex` query façade over the C ABI (include/rbq.h)."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _abi, _marshal
from ._abi import READ_FN, WRITE_FN  # noqa: F401  (their home is the prototype table; callers know them by this module)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
LIB_PATH = os.environ.get("RBQ_LIB_PATH") or os.path.join(_HERE, "csrc", "librbq.so")  # override: kernel A/B builds
RERANK_POOL_MAX = 4096  # largest pool of IvfRabitqIndex.set_rerank_pool (kRerankPoolMax: one workgroup orders a pool in LDS)


def _hip_runtime_of_torch_first():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so and asks for it by the
    unversioned name; librbq.so asks for libamdhip64.so.7.  If torch is loaded first, librbq.so binds to torch's copy
    (same SONAME) and the process has one runtime.  The other way round the loader maps a SECOND runtime for torch,
    which then sees no GPU ("No HIP GPUs are available": found by tests/diag/soak.py, whose first seed used this
    library before torch).  So when torch is installed it is imported before librbq.so is mapped; without torch
    (a C / Rust host, or a torch-less Python) there is only the system runtime and nothing to order."""
    import sys
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass


def lib():
    """Load csrc/librbq.so (HIP, gfx950). Fails loudly — there is no CPU fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} missing: the HIP extension must be built first "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        _hip_runtime_of_torch_first()
        _LIB = _abi.bind(C.CDLL(LIB_PATH), _abi.LIBRBQ)
    return _LIB


def _detail():
    buf = C.create_string_buffer(512)
    lib().rbq_last_error_detail(buf, 512)
    return buf.value.decode("utf-8", "replace")


def _check(rc):
    if rc != _abi.RBQ_OK:
        from . import RabitqError
        raise RabitqError(rc, _detail())


def _rescale(mode, t_const):
    """(RBQ_RESCALE_*, t_const as f32) for rescale="const" (RabitqConfig::faster) / "optimal" (RabitqConfig::new).
    An unknown mode is passed through as an integer the library rejects (InvalidConfig)."""
    m = _abi.RESCALE_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
    return m, float(t_const) if t_const is not None else 0.0


def _addr(ptr):
    return C.cast(ptr, C.c_void_p)


class IvfRabitqIndex:
    """Device-resident IVF+RaBitQ index; query methods mirror reference src/ivf.rs:1705-1752."""

    def __init__(self, handle, rescale=None):
        self._h = handle
        self._rescale = rescale  # (mode, t_const) the encoder ran with, where this object knows it: add()'s default
        self._range = None       # the radius set_range_search left on the handle (None: range search off)
        self._range_exact = None  # the exact radius set_range_exact left on the handle (None: off)

    # -- construction -------------------------------------------------------------
    @staticmethod
    def _devices(device, devices):
        """(n_devices, int array | None): `devices` = list of HIP ordinals (one replica each), else `device`."""
        if devices is not None:
            devices = list(devices)
            return len(devices), (C.c_int * len(devices))(*devices)
        return 1, ((C.c_int * 1)(device) if device is not None else None)

    @classmethod
    def from_built(cls, built, device=None, devices=None):
        """Upload a builder.BuiltIndex (ClusterData-shaped host arrays) with its reconstruction factors delta / vl
        (rbq_index_create_with_recon), so that the handle can be saved."""
        from . import builder
        h = C.c_void_p()
        n, dev = cls._devices(device, devices)
        nl = int(built.header.n_lists)
        fp = C.POINTER(C.c_float)
        delta, vl = (fp * nl)(), (fp * nl)()
        for c in range(nl):
            _check(builder.lib().rbq_built_list_recon(built._h, c, C.byref(delta[c]), C.byref(vl[c])))
        _check(lib().rbq_index_create_with_recon(_addr(built.hdr_ptr), _addr(built.lists_ptr), C.cast(delta, C.c_void_p),
                                                 C.cast(vl, C.c_void_p), n, dev, C.byref(h)))
        return cls(h)

    @classmethod
    def from_built_without_recon(cls, built, device=None, devices=None):
        """rbq_index_create: the same index without its reconstruction factors (it searches alike but cannot be saved)."""
        h = C.c_void_p()
        n, dev = cls._devices(device, devices)
        _check(lib().rbq_index_create(_addr(built.hdr_ptr), _addr(built.lists_ptr), n, dev, C.byref(h)))
        return cls(h)

    @classmethod
    def build_on_device(cls, hdr_ptr, centroids, d_data, d_assign, n, t_const=None, device=0, rescale="const"):
        """GPU-side encoder (rbq_index_build_device_ex): `hdr_ptr` is a ctypes pointer to an rbq_header (dim,
        padded_dim, metric, rotator + blob, ex_bits, n_lists), `centroids` a host [n_lists][dim] f32 array,
        `d_data` / `d_assign` device pointers to [n][dim] f32 vectors and [n] u32 cluster ids.
        rescale="const": RabitqConfig::faster, `t_const` for every vector (required unless 1-bit);
        rescale="optimal": RabitqConfig::new, every vector's own best_rescale_factor (`t_const` may be None)."""
        cent = np.ascontiguousarray(centroids, dtype=np.float32)
        mode, t = _rescale(rescale, t_const)
        h = C.c_void_p()
        _check(lib().rbq_index_build_device_ex(_addr(hdr_ptr), cent.ctypes.data, C.c_void_p(d_data), C.c_void_p(d_assign),
                                               int(n), mode, t, int(device), C.byref(h)))
        return cls(h, (rescale, t_const))

    @classmethod
    def train_on_device(cls, data, centroids, assignments, total_bits, metric, rotator_type, seed, use_faster_config,
                        device=0):
        """`train_with_clusters` (src/ivf.rs:1025-1215; the crate's Python `fit_with_clusters`) with the quantisation on
        the GPU.  The header — rotator, and t_const for the faster configuration — depends only on (dim, bits, seed), so
        it is taken from a CPU build over the first n_lists vectors; the whole set is then encoded on `device` with
        rescale "const" (use_faster_config) or "optimal".  `data` [n][dim] and `assignments` [n] are host arrays or
        CUDA tensors.  The index is identical, array for array, to the CPU build's."""
        import torch
        from . import RabitqError, builder
        dev = torch.device("cuda", int(device))
        xd = (data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)))
        xd = xd.to(device=dev, dtype=torch.float32).contiguous()
        ad = (assignments if isinstance(assignments, torch.Tensor) else torch.from_numpy(np.asarray(assignments).astype(np.int64)))
        ad = ad.to(device=dev, dtype=torch.int32).contiguous()
        cent = np.ascontiguousarray(centroids.cpu().numpy() if isinstance(centroids, torch.Tensor) else centroids, dtype=np.float32)
        if xd.dim() != 2 or ad.shape[0] != xd.shape[0] or cent.ndim != 2 or cent.shape[1] != xd.shape[1]:
            raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data [n][dim], assignments [n], centroids [n_lists][dim]")
        n, nlist = int(xd.shape[0]), int(cent.shape[0])
        if nlist == 0 or nlist > n:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "train_with_clusters needs 1 <= n_lists <= n")
        small = builder.train_with_clusters(xd[:nlist].cpu().numpy(), cent, np.arange(nlist, dtype=np.uint32), total_bits,
                                            metric, rotator_type, seed, True)
        try:
            return cls.build_on_device(small.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n,
                                       small.t_const if use_faster_config else None, device,
                                       "const" if use_faster_config else "optimal")
        finally:
            small.close()

    @classmethod
    def train(cls, data, nlist, total_bits, metric, rotator_type, seed, use_faster_config, device=0):
        """`IvfRabitqIndex::train` (src/ivf.rs:950-1021) end to end on `device`: the crate's checks and messages, k-means as
        `run_kmeans(data, nlist, 30, rng)` (seed = first draw of Rng(seed ^ 0x5a5a5a5a5a5a5a5a), the other KMeansConfig fields at
        their defaults) on the device, then train_on_device's rotation and quantisation (rescale "optimal" unless
        use_faster_config).  `data` [n][dim] is a host array or a CUDA tensor; it is uploaded once.  The index equals
        train_with_clusters over the CPU k-means restatement (builder.run_kmeans_with_config_cpu) with the same config."""
        from . import RabitqError
        from .kmeans import KMeansConfig, _run_device, first_draw, to_device
        shape = getattr(data, "shape", None)
        if shape is None or len(shape) == 0 or shape[0] == 0:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "training data must be non-empty")
        if nlist == 0:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "nlist must be positive")
        if total_bits == 0 or total_bits > 16:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "total_bits must be between 1 and 16")
        if len(shape) != 2:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "input vectors must share the same dimension")
        if nlist > shape[0]:
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "nlist cannot exceed number of vectors")
        xd = to_device(data, device)
        cfg = KMeansConfig(niter=30, seed=first_draw(int(seed) ^ 0x5A5A5A5A5A5A5A5A))
        cent, assign, _, _ = _run_device(xd, int(nlist), cfg, device)
        return cls.train_on_device(xd, cent, assign, total_bits, metric, rotator_type, seed, use_faster_config, device)

    @staticmethod
    def debug_best_rescale(o_abs, ex_bits, device=0):
        """Test hook (rbq_debug_best_rescale): best_rescale_factor of every row of o_abs [n][dim] (|r| / norm(r)),
        computed by the encoder's kernel; f64 [n]."""
        o = np.ascontiguousarray(o_abs, dtype=np.float32)
        out = np.empty(o.shape[0], np.float64)
        _check(lib().rbq_debug_best_rescale(o.ctypes.data, o.shape[0], o.shape[1], int(ex_bits), int(device), out.ctypes.data))
        return out

    def debug_copy_index(self, name, out):
        """Diagnostic: copy one of the index's device arrays into the numpy array `out` (exact size)."""
        _check(lib().rbq_debug_copy_index(self._h, name.encode(), out.ctypes.data, out.nbytes))
        return out

    @classmethod
    def load_from_bytes(cls, data, device=None, devices=None):
        """`load_from_reader` (src/ivf.rs:1484-1702) straight into HBM."""
        h = C.c_void_p()
        n, dev = cls._devices(device, devices)
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        _check(lib().rbq_index_load_rbq1(buf, len(data), n, dev, C.byref(h)))
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

    @classmethod
    def load_from_reader(cls, fileobj, device=None, devices=None):
        """`load_from_reader` over a binary file object (rbq_index_load_rbq1_stream): the stream runs from the object's
        current position to its end and is read span by span (at most 64 MB each) straight into the loader's page-locked
        buffers; the GPU checksums it and lays it out.  The index equals load_from_bytes' of the same bytes.  `fileobj`
        needs seek, tell and readinto (or read).  An exception raised by the file object stops the load and is re-raised."""
        start = fileobj.tell()
        fileobj.seek(0, os.SEEK_END)
        total = fileobj.tell() - start
        fn, err = _marshal.reader_callback(fileobj, start)
        h = C.c_void_p()
        n, dev = cls._devices(device, devices)
        rc = lib().rbq_index_load_rbq1_stream(fn, None, max(int(total), 0), n, dev, C.byref(h))
        if err:
            raise err[0]
        _check(rc)
        return cls(h)

    # -- persistence: save_to_writer (src/ivf.rs:1310-1474), bytes assembled on the device ------------------------
    def save_to_writer(self, fileobj):
        """Write the RBQ1 stream to `fileobj` (anything with .write(bytes)), chunk by chunk
        (rbq_index_save_rbq1_stream).  A writer exception stops the save and is re-raised."""
        fn, err = _marshal.writer_callback(fileobj)
        rc = lib().rbq_index_save_rbq1_stream(self._h, fn, None)
        if err:
            raise err[0]
        _check(rc)

    def save_to_bytes(self):
        """The whole RBQ1 stream as bytes (rbq_index_save_rbq1)."""
        return _marshal.owned_bytes(lambda p, n: _check(lib().rbq_index_save_rbq1(self._h, p, n)), lib().rbq_persist_free_bytes)

    def save_to_path(self, path):
        """save_to_path: the stream written to a file (created or truncated)."""
        try:
            f = open(path, "wb")
        except OSError as e:
            from . import RabitqError
            raise RabitqError(_abi.RBQ_IO, str(e))
        with f:
            self.save_to_writer(f)

    @staticmethod
    def debug_crc32_device(d_ptr, n, device=0):
        """Test hook (rbq_debug_crc32_device): CRC-32/IEEE of n device bytes at d_ptr, computed by the save path's kernels."""
        out = C.c_uint32()
        _check(lib().rbq_debug_crc32_device(C.c_void_p(d_ptr), int(n), int(device), C.byref(out)))
        return out.value

    # -- fetch_embedding (src/ivf.rs:1247-1307), decoded and inverse-rotated on the device ----------------------------
    def fetch_embeddings(self, ids):
        """rbq_index_fetch_embeddings: (out [n, dim] f32, found [n] bool).  Row i is the crate's fetch_embedding(ids[i]) bit
        for bit (the first occurrence in (cluster, position) order); a missing id gives a zero row and found False."""
        return _marshal.fetch_embeddings(lib().rbq_index_fetch_embeddings, self._h, self.dim, ids)

    def fetch_embedding(self, vector_id):
        """`IvfRabitqIndex::fetch_embedding`: the reconstructed vector [dim] f32, or None when the id is not in the index."""
        out, found = self.fetch_embeddings([vector_id])
        return out[0] if found[0] else None

    def fetch_embeddings_device(self, d_ids, n, d_out, d_found, stream=None):
        """rbq_index_fetch_embeddings_device: n u64 ids at d_ids (device memory of the first replica's device) -> d_out
        [n][dim] f32, d_found [n] u8, enqueued on `stream` (a hipStream_t as int, None = default stream)."""
        _marshal.fetch_embeddings_device(lib().rbq_index_fetch_embeddings_device, self._h, d_ids, n, d_out, d_found, stream)

    # -- growth (rbq_index_append) --------------------------------------------------------------------------------
    def id_bound(self):
        """1 + the largest stored id; 0 for an index without vectors (rbq_index_id_bound)."""
        out = C.c_uint64()
        _check(lib().rbq_index_id_bound(self._h, C.byref(out)))
        return int(out.value)

    def add(self, data, assignments=None, first_id=None, rescale=None, t_const=None, max_chunk_rows=0, devices=None):
        """FAISS-style add (rbq_index_append): the rows of `data` [count][dim] (a host array or a CUDA tensor) join the index with
        ids first_id .. (default: id_bound()), in the lists `assignments` [count] names (host array or CUDA tensor; None: the
        nearest rotated centroid of every row).  The index afterwards equals, array for array, a one-shot build over the old and
        the new rows.  rescale / t_const default to what train, train_on_device or build_on_device encoded this object with; a
        loaded object has to be given them.  The object's handle is swapped for the grown one (on `devices`, default the first
        replica's device) and the old one closed.  Returns the list of every row, [count] u32."""
        from . import RabitqError
        rescale, t_const = _marshal.known_rescale(self._rescale, rescale, t_const)
        xp, x = _marshal.rows_arg(data)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data must be [count][%d]" % self.dim)
        count = int(x.shape[0])
        ap = a = None
        if assignments is not None:
            torch = _marshal.torch_of(assignments)
            if torch is not None and assignments.is_cuda:
                a = assignments.to(dtype=torch.int32).contiguous()
                ap = C.c_void_p(a.data_ptr())
            else:
                a = np.ascontiguousarray(assignments.numpy() if torch is not None else assignments).astype(np.uint32)
                ap = C.c_void_p(a.ctypes.data)
            if a.ndim != 1 or a.shape[0] != count:
                raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "assignments must be [count]")
        mode, t = _rescale(rescale, t_const)
        out = np.empty(count, np.uint32)
        nd, dv = (1, None) if devices is None else self._devices(None, devices)
        h = C.c_void_p()
        _check(lib().rbq_index_append(self._h, xp, ap, count, self.id_bound() if first_id is None else int(first_id), mode, t,
                                      int(max_chunk_rows), nd, dv, out.ctypes.data, C.byref(h)))  # (x and a own what xp and ap name)
        self._rescale = (rescale, t_const)
        self._swap(h)
        return out

    def _swap(self, h):
        """The handle a mutation returned takes the place of the old one, which is closed."""
        old, self._h = self._h, h
        self._range = None  # (options are per handle: the new one starts with the range search off)
        self._range_exact = None
        lib().rbq_index_destroy(old)

    # -- shrinking (rbq_index_remove_ids) ------------------------------------------------------------------------------
    def remove_ids(self, ids, devices=None):
        """FAISS-style remove_ids (rbq_index_remove_ids): every stored vector whose id is in `ids` (a host array, a list, or a
        CUDA int64 / uint64 tensor; any order, repeats allowed, ids that are not stored ignored) leaves the index.  The index
        afterwards equals, array for array, a one-shot build over the rows that stay, with their original ids.  The object's handle
        is swapped for the shrunk one (on `devices`, default the first replica's device) and the old one closed; the remembered
        rescale mode stays.  Returns the number of slots removed; an empty `ids` returns 0 without a call."""
        n, p, _ids = _marshal.ids_arg(ids)  # (_ids owns what p names)
        if n == 0:
            return 0
        nd, dv = (1, None) if devices is None else self._devices(None, devices)
        h, removed = C.c_void_p(), C.c_uint64()
        _check(lib().rbq_index_remove_ids(self._h, p, n, nd, dv, C.byref(removed), C.byref(h)))
        self._swap(h)
        return int(removed.value)

    # -- accessors ----------------------------------------------------------------
    def __len__(self):
        return lib().rbq_index_len(self._h)

    def is_empty(self):
        return len(self) == 0

    def cluster_count(self):
        return lib().rbq_index_cluster_count(self._h)

    @property
    def dim(self):
        return lib().rbq_index_dim(self._h)

    @property
    def padded_dim(self):
        return lib().rbq_index_padded_dim(self._h)

    # -- queries ------------------------------------------------------------------
    def batch_search_raw(self, queries, params, filter_words=None, filter_nbits=0, want_diag=False, dtype=None):
        """Returns (ids[nq,k] u64, scores[nq,k] f32, counts[nq] u32, diag[nq,3] u64|None).
        `queries`: f32 rows, or 16-bit rows read as they are (option "query_dtype", set for this call): a numpy.float16 array, a
        torch.half / torch.bfloat16 tensor, or a numpy.uint16 array of bit patterns with dtype="f16" | "bf16" (_marshal.query_arg).
        A CUDA tensor takes rbq_search_batch_device on the current stream; the arrays come back on the host either way."""
        q, code = _marshal.query_arg(queries, dtype)
        if q.ndim == 1:
            q = q[None, :]
        nq, qd = q.shape
        k = params.top_k
        fw = np.ascontiguousarray(filter_words, dtype=np.uint32) if filter_words is not None else None
        if _marshal.on_device(q):
            return self._search_device_tensor(q, code, k, params.nprobe, fw, filter_nbits, want_diag)
        ids = np.empty((nq, k), np.uint64)
        scores = np.empty((nq, k), np.float32)
        counts = np.zeros(nq, np.uint32)
        diag = np.zeros((nq, 3), np.uint64) if want_diag else None
        with self._query_dtype_for_call(code):
            rc = lib().rbq_search_batch(self._h, _marshal.data_ptr(q), nq, qd, k, params.nprobe,
                                        fw.ctypes.data if fw is not None else None, filter_nbits,
                                        ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                        diag.ctypes.data if diag is not None else None)
        _check(rc)
        return ids, scores, counts, diag

    def _search_device_tensor(self, q, code, k, nprobe, fw, filter_nbits, want_diag):
        """batch_search_raw for a CUDA tensor: the device entry on the tensor's current stream, results copied to the host."""
        import torch
        nq, qd = q.shape
        with torch.cuda.device(q.device):
            ids = torch.empty((nq, max(k, 1)), dtype=torch.int64, device=q.device)
            sc = torch.empty((nq, max(k, 1)), dtype=torch.float32, device=q.device)
            cnt = torch.zeros(nq, dtype=torch.int32, device=q.device)
            dg = torch.zeros((nq, 3), dtype=torch.int64, device=q.device) if want_diag else None
            dfw = torch.from_numpy(fw.view(np.int32)).to(q.device) if fw is not None else None
            st = torch.cuda.current_stream()
            with self._query_dtype_for_call(code):
                self.search_batch_device(q.data_ptr(), nq, qd, k, nprobe, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(),
                                         stream=C.c_void_p(st.cuda_stream), d_filter=dfw.data_ptr() if dfw is not None else None,
                                         filter_nbits=filter_nbits, d_diag=dg.data_ptr() if dg is not None else None)
            st.synchronize()
        return (ids.cpu().numpy().view(np.uint64)[:, :k], sc.cpu().numpy()[:, :k], cnt.cpu().numpy().view(np.uint32),
                dg.cpu().numpy().view(np.uint64) if dg is not None else None)

    # -- 16-bit queries (option "query_dtype") ------------------------------------------------------
    def set_query_dtype(self, dtype):
        """What every entry point of this handle reads its query pointer as from now on: "f32" (default), "f16" or "bf16" (or
        RBQ_RAW_*) - rows of `dim` elements, 2 * dim bytes apart for the 16-bit types, widened exactly where a kernel loads
        them.  For callers that pass raw pointers (search_batch_device, range_search_device, the device entries of MSTG); the
        array-taking methods set it for the call from the array's own type and put this value back.  None: "f32"."""
        if dtype is None:
            dtype = _abi.RAW_F32
        if isinstance(dtype, str):
            if dtype not in _abi.RAW_DTYPES:
                from . import RabitqError
                raise RabitqError(_abi.RBQ_INVALID_CONFIG, "unknown query dtype %r (one of %s)" % (dtype, ", ".join(_abi.RAW_DTYPES)))
            dtype = _abi.RAW_DTYPES[dtype]
        self.set_option("query_dtype", int(dtype))

    def _query_dtype_code(self):
        v = C.c_int32(-1)
        _check(lib().rbq_debug_copy_index(self._h, b"query_dtype", C.byref(v), 4))
        return int(v.value)

    def query_dtype(self):
        """"f32" / "f16" / "bf16": the option "query_dtype" as the handle holds it."""
        return {i: n for n, i in _abi.RAW_DTYPES.items()}[self._query_dtype_code()]

    @contextlib.contextmanager
    def _query_dtype_for_call(self, code):
        """Context of one call whose queries are of type `code`: the option is set where it differs from what the HANDLE holds
        (read back from it: set_option("query_dtype", ...) and set_query_dtype are one and the same to this) and the handle's
        value put back afterwards, error or not.  f32 input on a handle at f32 makes no option call."""
        before = self._query_dtype_code()
        if code == before:
            yield
            return
        self.set_option("query_dtype", code)
        try:
            yield
        finally:
            self.set_option("query_dtype", before)

    def _results(self, ids, scores, counts, q):
        from . import SearchResult
        return [SearchResult(int(ids[q, i]), float(scores[q, i])) for i in range(int(counts[q]))]

    def search(self, query, params, dtype=None):
        """`IvfRabitqIndex::search` (src/ivf.rs:1705-1711)."""
        ids, scores, counts, _ = self.batch_search_raw(query, params, dtype=dtype)
        return self._results(ids, scores, counts, 0)

    def search_filtered(self, query, params, allowed_ids, dtype=None):
        """`search_filtered` (src/ivf.rs:1723-1730); `allowed_ids` plays the RoaringBitmap."""
        allowed = np.asarray(sorted(set(int(i) for i in allowed_ids)), dtype=np.uint64)
        nbits = int(allowed.max()) + 1 if allowed.size else 0
        words = np.zeros((nbits + 31) // 32 or 1, np.uint32)
        if allowed.size:
            np.bitwise_or.at(words, (allowed >> np.uint64(5)).astype(np.int64),
                             (np.uint32(1) << (allowed & np.uint64(31)).astype(np.uint32)))
        ids, scores, counts, _ = self.batch_search_raw(query, params, words, nbits, dtype=dtype)
        return self._results(ids, scores, counts, 0)

    def batch_search(self, queries, params, dtype=None):
        """`batch_search` (src/ivf.rs:1743-1752): per-query results in input order."""
        ids, scores, counts, _ = self.batch_search_raw(queries, params, dtype=dtype)
        return [self._results(ids, scores, counts, q) for q in range(ids.shape[0])]

    def batch_query(self, queries, top_k, nprobe, dtype=None):
        """Python-binding shape of the reference (`batch_query`, src/python_bindings.rs:593-665):
        list of (k,2) f32 arrays [id, score] (ids cast to f32 exactly as the reference does)."""
        from . import SearchParams
        ids, scores, counts, _ = self.batch_search_raw(queries, SearchParams(top_k, nprobe), dtype=dtype)
        out = []
        for q in range(ids.shape[0]):
            c = int(counts[q])
            out.append(np.stack([ids[q, :c].astype(np.float32), scores[q, :c]], axis=1))
        return out

    def posting_scan(self, queries, top_k, list_ids, list_counts, dtype=None):
        """MSTG posting-list scan (reference src/mstg/index.rs:149-330): the caller has already chosen each
        query's posting lists. Returns (ids[nq,k] u64, distances[nq,k] f32 ascending, counts[nq] u32).
        `queries` (host) and `dtype` as batch_search_raw."""
        from . import RabitqError
        q, code = _marshal.query_arg(queries, dtype)
        if _marshal.on_device(q):
            raise RabitqError(_abi.RBQ_INVALID_CONFIG, "posting_scan takes host queries")
        li = np.ascontiguousarray(list_ids, dtype=np.uint32)
        lc = np.ascontiguousarray(list_counts, dtype=np.uint32)
        nq, qd = q.shape
        ids = np.empty((nq, top_k), np.uint64)
        scores = np.empty((nq, top_k), np.float32)
        counts = np.zeros(nq, np.uint32)
        with self._query_dtype_for_call(code):
            rc = lib().rbq_posting_scan_batch(self._h, _marshal.data_ptr(q), nq, qd, top_k, li.ctypes.data, lc.ctypes.data,
                                              li.shape[1], ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
        _check(rc)
        return ids, scores, counts

    # -- device-pointer entry (bench / torch interop) --------------------------------
    def search_batch_device(self, d_queries, nq, query_dim, top_k, nprobe, d_ids, d_scores, d_counts,
                            stream=None, d_filter=None, filter_nbits=0, d_diag=None):
        _check(lib().rbq_search_batch_device(self._h, d_queries, nq, query_dim, top_k, nprobe, d_filter,
                                             filter_nbits, d_ids, d_scores, d_counts, d_diag, stream))

    # -- range search: every probed vector within a radius ------------------------------------
    def set_range_search(self, radius):
        """Options "range_radius_bits" / "range_search": with a radius (any f32, passed by its bits), batch_search_raw and
        search_batch_device return, per query, every vector of the probed lists with distance < radius (L2) or score > radius
        (inner product), in scan order (probe order, then position inside the list): top_k is the capacity of the row,
        counts the TOTAL number of matches (it may exceed the capacity), unused slots are UINT64_MAX / NaN.  None switches
        it off and puts the radius back to +inf."""
        if radius is None:
            self.set_option("range_search", 0)
            self.set_option("range_radius_bits", 0x7F800000)
        else:
            self.set_option("range_radius_bits", int(np.array([radius], np.float32).view(np.int32)[0]))
            self.set_option("range_search", 1)
        self._range = radius

    # -- exact range search: the estimate's matches are candidates, the raw vectors decide --------
    def set_range_exact(self, exact_radius):
        """Options "range_exact_radius_bits" / "range_exact": with an exact radius x (any f32, passed by its bits), a range
        search (set_range_search) on a handle with raw vectors attached (set_rerank_vectors) treats the estimate's matches at
        its own radius as candidates, scores each exactly against its raw row and returns those with exact distance < x (L2)
        or exact dot product > x (inner product), in scan order with their exact scores.  None switches it off and puts x
        back to +inf.  Without raw vectors attached (or with the option "rerank" 0) the search then raises InvalidConfig."""
        if exact_radius is None:
            self.set_option("range_exact", 0)
            self.set_option("range_exact_radius_bits", 0x7F800000)
        else:
            self.set_option("range_exact_radius_bits", int(np.array([exact_radius], np.float32).view(np.int32)[0]))
            self.set_option("range_exact", 1)
        self._range_exact = exact_radius

    @contextlib.contextmanager
    def _range_for_call(self, radius, exact, candidate_radius):
        """The range options of one call, put back afterwards, error or not.  exact=False: `radius` is the estimate's.
        exact=True: `radius` is the exact radius x and `candidate_radius` the estimate's r (None: +inf for L2, -inf for inner
        product — every probed vector is a candidate)."""
        from . import RabitqError
        before, before_x = getattr(self, "_range", None), getattr(self, "_range_exact", None)
        if exact:
            if candidate_radius is None:
                m = np.full(1, -1, np.int32)
                _check(lib().rbq_debug_copy_index(self._h, b"metric", m.ctypes.data, 4))
                candidate_radius = np.float32(np.inf) if int(m[0]) == 0 else np.float32(-np.inf)
            r, x = candidate_radius, radius
        else:
            if candidate_radius is not None:
                raise RabitqError(_abi.RBQ_INVALID_CONFIG, "candidate_radius goes with exact=True")
            r, x = radius, None
        touch_x = exact or before_x is not None  # (a plain call on a handle that never had range_exact on sets nothing more than before)
        try:
            if touch_x:
                self.set_range_exact(x)
            self.set_range_search(r)
            yield
        finally:
            self.set_range_search(before)
            if touch_x:
                self.set_range_exact(before_x)

    @staticmethod
    def _filter_words(allowed_ids):
        allowed = np.asarray(sorted(set(int(i) for i in allowed_ids)), dtype=np.uint64)
        nbits = int(allowed.max()) + 1 if allowed.size else 0
        words = np.zeros((nbits + 31) // 32 or 1, np.uint32)
        if allowed.size:
            np.bitwise_or.at(words, (allowed >> np.uint64(5)).astype(np.int64),
                             (np.uint32(1) << (allowed & np.uint64(31)).astype(np.uint32)))
        return words, nbits

    @staticmethod
    def _range_csr(ids, scores, counts, sort):
        """Rows of capacity cap with their totals -> FAISS's (lims [nq + 1], ids, scores); a row holds min(total, cap)."""
        kept = np.minimum(counts.astype(np.int64), ids.shape[1])
        lims = np.zeros(len(kept) + 1, np.int64)
        np.cumsum(kept, out=lims[1:])
        take = np.arange(ids.shape[1])[None, :] < kept[:, None]
        out_ids, out_sc = ids[take], scores[take]  # (row-major: rows in query order, scan order inside a row)
        if sort:
            for q in range(len(kept)):
                o = np.argsort(out_sc[lims[q]:lims[q + 1]], kind="stable")  # (score, scan order)
                out_ids[lims[q]:lims[q + 1]] = out_ids[lims[q]:lims[q + 1]][o]
                out_sc[lims[q]:lims[q + 1]] = out_sc[lims[q]:lims[q + 1]][o]
        return lims, out_ids, out_sc

    def range_search(self, queries, radius, nprobe, max_results=None, allowed_ids=None, want_diag=False, sort=False, dtype=None,
                     exact=False, candidate_radius=None):
        """FAISS-style range_search over the probed lists: (lims [nq + 1] i64, ids u64, scores f32) — query q's matches are
        ids[lims[q]:lims[q + 1]], in scan order, or ascending by (score, scan order) with sort=True.  A match has distance <
        radius (L2) or score > radius (inner product).  max_results=None: complete rows (a first call with rows of 1024; where
        a total exceeds that, one more with rows of the largest total — the totals are exact, so one repeat suffices).
        max_results=m: at most the first m matches of every query, and the totals [nq] u32 as a fourth value.  want_diag: the
        SearchDiagnostics [nq, 3] u64 as the last value.  `allowed_ids` as search_filtered.  The handle's range options are
        set for the call and put back afterwards.  `queries` and `dtype` as batch_search_raw.
        exact=True (raw vectors attached with set_rerank_vectors): `radius` is the EXACT radius x — a match has exact distance <
        x (L2) or exact dot product > x (inner product), and the scores returned are exact — and `candidate_radius` is the
        estimate's radius r that picks the candidates to score (set_range_exact).  candidate_radius=None: +inf (L2) / -inf
        (inner product), every probed vector — complete over the probed lists, slow, and the default because it is the one that
        cannot lose a match.  The diagnostics are those of the candidate scan."""
        from . import SearchParams
        queries, dtype = _marshal.query_arg(queries, dtype)
        words, nbits = self._filter_words(allowed_ids) if allowed_ids is not None else (None, 0)
        cap = max_results or 1024
        with self._range_for_call(radius, exact, candidate_radius):
            ids, sc, cnt, diag = self.batch_search_raw(queries, SearchParams(cap, nprobe), words, nbits, want_diag, dtype)
            if max_results is None and cnt.size and int(cnt.max()) > cap:
                ids, sc, cnt, diag = self.batch_search_raw(queries, SearchParams(int(cnt.max()), nprobe), words, nbits, want_diag, dtype)
        out = self._range_csr(ids, sc, cnt, sort)
        if max_results is not None:
            out += (cnt,)
        return out + (diag,) if want_diag else out

    def range_search_device(self, d_queries, nq, query_dim, radius, nprobe, cap, d_ids, d_scores, d_counts, stream=None,
                            d_filter=None, filter_nbits=0, d_diag=None, exact=False, candidate_radius=None):
        """range_search on device pointers (search_batch_device with the range options set for the call): rows of capacity
        `cap` at d_ids / d_scores, the totals at d_counts, enqueued on `stream` without host synchronisation.  The caller
        reads d_counts once the stream has got there and repeats with a larger `cap` where a total exceeds it.
        `exact` / `candidate_radius` as range_search."""
        with self._range_for_call(radius, exact, candidate_radius):
            self.search_batch_device(d_queries, nq, query_dim, cap, nprobe, d_ids, d_scores, d_counts, stream, d_filter,
                                     filter_nbits, d_diag)

    def profile_begin(self, stages=("prep", "rank", "select", "scan"), every=1):
        mask = sum(1 << ("prep", "rank", "select", "scan").index(s) for s in stages)
        lib().rbq_profile_select_stages(self._h, mask)
        lib().rbq_profile_set_sampling(self._h, every)
        lib().rbq_profile_begin(self._h)

    def profile_end(self):
        lib().rbq_profile_end(self._h)

    def profile_stage(self, name):
        n = C.c_uint64()
        ms = lib().rbq_profile_stage_ms(self._h, name.encode(), C.byref(n))
        return ms, n.value

    def profile_stage_samples(self, name):
        """durations (ms) of the individual timed launches of a stage between profile_begin/end"""
        n = lib().rbq_profile_stage_samples(self._h, name.encode(), None, 0)
        out = np.zeros(max(int(n), 1), np.float32)
        lib().rbq_profile_stage_samples(self._h, name.encode(), out.ctypes.data, int(n))
        return out[:int(n)]

    def set_option(self, name, value):
        _check(lib().rbq_debug_set_option(self._h, name.encode(), int(value)))

    def set_numeric_variant(self, variant):
        """Which build of the reference the scores reproduce bit for bit: "native_avx512" (default: the crate built in its own
        checkout on an AVX-512 host), "native_avx2" (the same on an AVX2-only host) or "portable" (RUSTFLAGS="" builds: crates.io
        dependents, the PyPI wheel).  An int is passed through as RBQ_NUMERIC_* (anything else is rejected by the library)."""
        if isinstance(variant, str):
            if variant not in _abi.NUMERIC_VARIANTS:
                from . import RabitqError
                raise RabitqError(_abi.RBQ_INVALID_CONFIG, "unknown numeric variant %r (one of %s)" % (variant, ", ".join(_abi.NUMERIC_VARIANTS)))
            variant = _abi.NUMERIC_VARIANTS[variant]
        _check(lib().rbq_index_set_numeric_variant(self._h, int(variant)))

    @property
    def numeric_variant(self):
        """The current numeric variant by name ("native_avx512", "native_avx2" or "portable")."""
        v = lib().rbq_index_numeric_variant(self._h)
        return {i: n for n, i in _abi.NUMERIC_VARIANTS.items()}[v]

    def stage_resources(self, nq, top_k, nprobe):
        """{stage: {workgroups, threads, vgprs, lds_bytes, scratch_bytes}} of the kernels a call of this shape launches (nothing runs);
        the rank stage also names its operand format: "operands" is "bf16x3", "f16" or "f32" there"""
        out = np.zeros((4, 6), np.uint32)
        _check(lib().rbq_debug_stage_resources(self._h, nq, top_k, nprobe, out.ctypes.data))
        res = {s: {"workgroups": int(o[0]), "threads": int(o[1]), "vgprs": int(o[2]), "lds_bytes": int(o[3]), "scratch_bytes": int(o[4])}
               for s, o in zip(("prep", "rank", "select", "scan"), out)}
        # what the ranking stage multiplies: three split-bf16 products, one f16 product, or f32 (the f32 GEMM and the exact scorers)
        res["rank"]["operands"] = {1: "bf16x3", 2: "f16", 3: "f32"}[int(out[1][5])]
        return res

    def head_exact_stats(self):
        """(queries whose probe selection ran the exact head evaluation, guard trips — must be 0)"""
        return int(lib().rbq_debug_head_exact_evaluations(self._h)), int(lib().rbq_debug_head_exact_guard_trips(self._h))

    def tie_log_stats(self):
        """k_scan's tie log: {replays, entries, heap_ops, overflows} since the index was created"""
        out = np.zeros(4, np.uint64)
        lib().rbq_debug_tie_log_stats(self._h, out.ctypes.data)
        return dict(zip(("replays", "entries", "heap_ops", "overflows"), (int(v) for v in out)))

    def rank_fallbacks(self):
        return lib().rbq_debug_rank_fallbacks(self._h)

    def debug_copy_workspace(self, stream, name, out):
        """Diagnostic: copy an intermediate device buffer of `stream`'s workspace into the numpy array `out`."""
        _check(lib().rbq_debug_copy_workspace(self._h, C.c_void_p(stream), name.encode(), out.ctypes.data, out.nbytes))
        return out

    def heap_restarts(self):
        return lib().rbq_debug_heap_restarts(self._h)

    def profile_scan_bytes(self):
        return lib().rbq_profile_scan_bytes(self._h)

    def device_count(self):
        return lib().rbq_index_device_count(self._h)

    def profile_counters(self):
        """dict of the scan's traffic counters between profile_begin/end (rbq_profile_counters)."""
        out = (C.c_uint64 * 8)()
        _check(lib().rbq_profile_counters(self._h, out, 8))
        names = ("vectors_probed", "code_blocks", "meta_blocks", "stream_entries", "ex_evals", "queries")
        return {k: int(out[i]) for i, k in enumerate(names)}

    def release_stream(self, stream):
        _check(lib().rbq_release_stream(self._h, C.c_void_p(stream)))

    def set_rerank_vectors(self, vectors=None, device_ptr=None, n=0, pool=None, dtype=None):
        """OPTIONAL extension (default off, not reference behaviour): attach raw vectors for the exact rerank.
        `vectors` = host array [n][dim], or `device_ptr` + n; None detaches.  `pool` (not None): set_rerank_pool(pool)
        once the vectors are attached.
        `dtype`: the element type the rows are kept in, "f32", "f16" or "bf16" (or RBQ_RAW_*).  16-bit rows take half the bytes
        and are widened exactly where they are scored: the results are those of the widened rows attached as f32.
        None: a numpy.float16 array attaches as f16, anything else as f32 (as before).  With `device_ptr` it says what the
        pointer holds.  "f16" with a host array of another type converts with astype(numpy.float16) (round to nearest even: the
        caller's choice, and the caller's recall); "bf16" with a host array takes a uint16 array of bit patterns (NumPy has no
        bf16; the library never rounds)."""
        from . import RabitqError
        if dtype is None:
            code = _abi.RAW_F16 if (device_ptr is None and isinstance(vectors, np.ndarray) and vectors.dtype == np.float16) else _abi.RAW_F32
        elif isinstance(dtype, str):
            if dtype not in _abi.RAW_DTYPES:
                raise RabitqError(_abi.RBQ_INVALID_CONFIG, "unknown rerank dtype %r (one of %s)" % (dtype, ", ".join(_abi.RAW_DTYPES)))
            code = _abi.RAW_DTYPES[dtype]
        else:
            code = int(dtype)
        if device_ptr is not None or vectors is not None:  # what the next attach reads its pointer as (option "rerank_raw_dtype")
            self.set_option("rerank_raw_dtype", code)
        if device_ptr is not None:
            _check(lib().rbq_index_set_rerank_vectors(self._h, C.c_void_p(device_ptr), int(n)))
        elif vectors is None:
            _check(lib().rbq_index_set_rerank_vectors(self._h, None, 0))
        else:
            if code == _abi.RAW_BF16:
                if not (isinstance(vectors, np.ndarray) and vectors.dtype == np.uint16):
                    raise RabitqError(_abi.RBQ_INVALID_CONFIG, "bf16 rows on the host are a uint16 array of bit patterns")
                v = np.ascontiguousarray(vectors)
            else:
                v = np.ascontiguousarray(vectors, dtype=np.float16 if code == _abi.RAW_F16 else np.float32)
            _check(lib().rbq_index_set_rerank_vectors(self._h, v.ctypes.data, v.shape[0]))
        if pool is not None:
            self.set_rerank_pool(pool)

    def rerank_dtype(self):
        """"f32" / "f16" / "bf16": the element type of the attached rerank vectors; None with nothing attached."""
        v = np.full(1, -1, np.int32)
        _check(lib().rbq_debug_copy_index(self._h, b"rerank_raw_dtype", v.ctypes.data, 4))
        return {i: n for n, i in _abi.RAW_DTYPES.items()}.get(int(v[0]))

    def set_rerank_pool(self, n):
        """Candidates the rerank re-scores per query (option "rerank_pool", at most RERANK_POOL_MAX): while raw vectors are
        attached and n > top_k, a search takes its n best candidates by the estimate, scores them exactly and returns the
        best top_k.  None or 0 switches it off: the rerank then re-scores the top_k returned ids only."""
        self.set_option("rerank_pool", 0 if n is None else int(n))

    def close(self):
        if self._h:
            lib().rbq_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamBuilder:
    """Streamed GPU-side encoder (rbq_build_stream_*): `train_with_clusters` (src/ivf.rs:1025-1215) with the
    vectors delivered chunk by chunk, for data sets that do not fit in HBM at once."""

    def __init__(self, hdr_ptr, centroids, list_sizes, t_const=None, device=0, rescale="const"):
        """rescale as for IvfRabitqIndex.build_on_device ("const": t_const; "optimal": per-vector factor)."""
        cent = np.ascontiguousarray(centroids, dtype=np.float32)
        ls = np.ascontiguousarray(list_sizes, dtype=np.uint32)
        mode, t = _rescale(rescale, t_const)
        self._b = C.c_void_p()
        _check(lib().rbq_build_stream_begin_ex(_addr(hdr_ptr), cent.ctypes.data, ls.ctypes.data, mode, t, int(device),
                                               C.byref(self._b)))

    def push(self, vectors, assign, first_id, count=None):
        """vectors / assign: numpy arrays (host) or integer device pointers (then `count` is required)."""
        if isinstance(vectors, np.ndarray):
            v = np.ascontiguousarray(vectors, dtype=np.float32)
            a = np.ascontiguousarray(assign, dtype=np.uint32)
            _check(lib().rbq_build_stream_push(self._b, v.ctypes.data, a.ctypes.data, int(first_id), v.shape[0]))
        else:
            _check(lib().rbq_build_stream_push(self._b, C.c_void_p(vectors), C.c_void_p(assign), int(first_id), int(count)))

    def finish(self, devices=None):
        h = C.c_void_p()
        if devices is None:
            _check(lib().rbq_build_stream_finish(self._b, 1, None, C.byref(h)))
        else:
            devices = list(devices)
            _check(lib().rbq_build_stream_finish(self._b, len(devices), (C.c_int * len(devices))(*devices), C.byref(h)))
        self._b = None
        return IvfRabitqIndex(h)

    def abort(self):
        if self._b:
            lib().rbq_build_stream_abort(self._b)
            self._b = None

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass
