"""CPU index builder (train-time harness) — ctypes binding of csrc/host/rbq_build.cpp.

Mirrors `IvfRabitqIndex::train_with_clusters` (reference src/ivf.rs:1025-1103). Training
stays on the CPU; the result is the reference's `ClusterData` byte layout, ready for
rbq_index_create (GPU) or for serialisation as RBQ1 v3."""
import ctypes as C
import os

import numpy as np

from ._abi import BF_FACTORS, LIBRBQ_BUILD, ROTATOR_FHT_KAC, RBQ_OK, MstgConfig, bind
from ._marshal import owned_bytes

# the device library's message for a padded_dim that is not a multiple of 16 (validate_header); the CPU builders return only the code
NOT_MULTIPLE_OF_16 = "Dimension must be multiple of 16 for SIMD"

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("RBQ_BUILD_LIB") or os.path.join(_HERE, "csrc", "librbq_build.so")  # (override: the sanitizer build)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _LIB = bind(C.CDLL(path), LIBRBQ_BUILD)
    return _LIB


HCLUSTER_STATS = ("splits", "balance_moves", "empty_reseeded", "rng_draws", "host_splits", "arena_bytes")


def take_hclustered(L, h, n, dim):
    """(centroids [count][dim] f32, offsets [count + 1] u64, members [n] u32, stats dict) copied out of the handle, which is freed."""
    try:
        cnt = int(L.rbq_hclustered_count(h))
        cent = np.ctypeslib.as_array(L.rbq_hclustered_centroids(h), shape=(cnt, dim)).copy() if cnt else np.zeros((0, dim), np.float32)
        off = np.ctypeslib.as_array(L.rbq_hclustered_offsets(h), shape=(cnt + 1,)).copy()
        mem = np.ctypeslib.as_array(L.rbq_hclustered_members(h), shape=(n,)).copy()
        st = dict(zip(HCLUSTER_STATS, (int(L.rbq_hclustered_stats(h)[i]) for i in range(len(HCLUSTER_STATS)))))
    finally:
        L.rbq_hclustered_free(h)
    return cent, off, mem, st


class BuiltIndex:
    """Host-resident index in the reference's ClusterData layout."""

    def __init__(self, handle):
        self._h = handle
        self.hdr_ptr = lib().rbq_built_header(handle)
        self.lists_ptr = lib().rbq_built_lists(handle)

    @property
    def header(self):
        return self.hdr_ptr.contents

    @property
    def hdr(self):
        return self.hdr_ptr.contents

    @property
    def t_const(self):
        """Constant rescale factor of the faster config (0.0 when it was not used)."""
        return float(lib().rbq_built_t_const(self._h))

    @property
    def dim(self):
        return self.header.dim

    @property
    def padded_dim(self):
        return self.header.padded_dim

    @property
    def n_lists(self):
        return self.header.n_lists

    def __len__(self):
        return self.header.n_vectors

    def list_sizes(self):
        return np.array([self.lists_ptr[i].n for i in range(self.n_lists)], dtype=np.int64)

    def list_ids(self, c):
        lv = self.lists_ptr[c]
        return np.ctypeslib.as_array(lv.ids, shape=(lv.n,)).copy() if lv.n else np.zeros(0, np.uint64)

    def centroid(self, c):
        return np.ctypeslib.as_array(self.lists_ptr[c].centroid, shape=(self.padded_dim,)).copy()

    def list_arrays(self, c):
        """Every array of ClusterData c (src/ivf.rs:205-242) as numpy copies: centroid, ids, batch_data, ex_codes [n][D*ex/8],
        f_add_ex, f_rescale_ex, delta, vl."""
        lv = self.lists_ptr[c]
        n, D, ex = int(lv.n), int(self.padded_dim), int(self.header.ex_bits)
        exb = D * ex // 8
        arr = lambda p, shape, dt: (np.ctypeslib.as_array(p, shape=shape).copy() if shape[0] else np.zeros(shape, dt))  # noqa: E731
        d, v = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        assert lib().rbq_built_list_recon(self._h, c, C.byref(d), C.byref(v)) == RBQ_OK
        return {"centroid": self.centroid(c), "ids": self.list_ids(c),
                "batch_data": arr(lv.batch_data, (int(lv.batch_len),), np.uint8),
                "ex_codes": arr(lv.ex_codes, (n, exb), np.uint8) if exb and n else np.zeros((n, exb), np.uint8),
                "f_add_ex": arr(lv.f_add_ex, (n,), np.float32), "f_rescale_ex": arr(lv.f_rescale_ex, (n,), np.float32),
                "delta": arr(d, (n,), np.float32), "vl": arr(v, (n,), np.float32)}

    def list_residual_norm(self, c):
        """QuantizedVector::residual_norm of list c's vectors (what the `.mstg` format stores next to the other factors)."""
        n = int(self.lists_ptr[c].n)
        p = C.POINTER(C.c_float)()
        assert lib().rbq_built_list_residual_norm(self._h, c, C.byref(p)) == RBQ_OK
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.float32)

    def rotator_blob(self):
        h = self.header
        return bytes(np.ctypeslib.as_array(h.rotator_blob, shape=(int(h.rotator_len),))) if h.rotator_len else b""

    def rotate(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.padded_dim, np.float32)
        lib().rbq_build_rotate(self.hdr_ptr, x.ctypes.data, out.ctypes.data)
        return out

    def save_rbq1(self):
        def call(p, n):
            assert lib().rbq_built_save_rbq1(self._h, p, n) == RBQ_OK
        return owned_bytes(call, lib().rbq_build_free_bytes)

    def close(self):
        if self._h:
            lib().rbq_built_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_with_clusters(data, centroids, assignments, total_bits, metric, rotator_type, seed,
                        use_faster_config):
    data = np.ascontiguousarray(data, dtype=np.float32)
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    assignments = np.ascontiguousarray(assignments, dtype=np.uint32)
    n, dim = data.shape
    h = C.c_void_p()
    rc = lib().rbq_build_train_with_clusters(
        data.ctypes.data, n, dim, centroids.ctypes.data, centroids.shape[0], assignments.ctypes.data,
        total_bits, metric, rotator_type, seed, int(use_faster_config), C.byref(h))
    if rc != RBQ_OK:
        from . import RabitqError
        raise RabitqError(rc, NOT_MULTIPLE_OF_16 if rotator_type != ROTATOR_FHT_KAC and dim % 16 else
                          "train_with_clusters rejected its configuration")
    return BuiltIndex(h)


def mstg_file_check(data):
    """The `.mstg` loader's validation on the CPU (rbq_build_mstg_file_check): (code, detail, config dict or None, info dict or
    None) — framing, every record's inner fields and the checksum, as rbq_mstg_load refuses or accepts them."""
    data = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))  # an exact-size heap copy: a read past the end is a sanitizer report
    detail = C.create_string_buffer(512)
    cfg = MstgConfig()
    out = np.zeros(4, np.uint64)
    rc = lib().rbq_build_mstg_file_check(data, len(data), detail, 512, C.byref(cfg), out.ctypes.data)
    if rc != RBQ_OK:
        return rc, detail.value.decode(), None, None
    return rc, "", cfg.to_dict(), dict(zip(("lists", "vectors", "dim", "ex_bits"), (int(v) for v in out)))


def best_rescale_factor(o_abs, ex_bits):
    """best_rescale_factor (src/quantizer.rs:337-427) of one vector, o_abs [dim] = |r_i| / norm(r) (the CPU reference)."""
    o = np.ascontiguousarray(o_abs, dtype=np.float32)
    return float(lib().rbq_build_best_rescale_factor(o.ctypes.data, o.shape[0], int(ex_bits)))


def kmeans(data, k, iters=10, seed=0):
    data = np.ascontiguousarray(data, dtype=np.float32)
    n, dim = data.shape
    cent = np.empty((k, dim), np.float32)
    assign = np.empty(n, np.uint32)
    rc = lib().rbq_build_kmeans(data.ctypes.data, n, dim, k, iters, seed, cent.ctypes.data, assign.ctypes.data)
    assert rc == RBQ_OK
    return cent, assign


def train(data, nlist, total_bits, metric, rotator_type, seed, use_faster_config, kmeans_iters=10):
    """`IvfRabitqIndex::train` (src/ivf.rs:950-1021) with a plain Lloyd k-means harness."""
    cent, assign = kmeans(data, nlist, kmeans_iters, seed ^ 0x5A5A5A5A5A5A5A5A)
    return train_with_clusters(data, cent, assign, total_bits, metric, rotator_type, seed, use_faster_config)


def run_kmeans_with_config_cpu(data, k, config=None, stats=None):
    """`run_kmeans_with_config` (src/kmeans.rs) in the pinned arithmetic of rbq_build.cpp, on the CPU: the specification the
    GPU k-means (kmeans.run_kmeans_with_config) equals bit for bit.  `stats`, when a dict, receives empty_reseeded and rng_draws."""
    from .kmeans import KMeansResult, _args, validate
    data = np.ascontiguousarray(data, dtype=np.float32)
    if data.ndim != 2:
        from . import RabitqError
        from ._abi import RBQ_DIMENSION_MISMATCH
        raise RabitqError(RBQ_DIMENSION_MISMATCH, "data must be [n][dim]")
    n, dim = data.shape
    validate(n, dim, int(k), config, lambda: bool(np.isfinite(data).all()))
    niter, nredo, seed, sph, mppc, dbs = _args(config)
    cent = np.empty((int(k), dim), np.float32)
    assign = np.empty(n, np.uint32)
    obj = C.c_double()
    st = np.zeros(2, np.uint64)
    rc = lib().rbq_build_kmeans_faiss(data.ctypes.data, n, dim, int(k), niter, nredo, seed, sph, mppc, dbs, cent.ctypes.data,
                                      assign.ctypes.data, C.byref(obj), st.ctypes.data)
    if rc != RBQ_OK:
        from . import RabitqError
        raise RabitqError(rc, "run_kmeans_with_config rejected its configuration")
    if stats is not None:
        stats.update(empty_reseeded=int(st[0]), rng_draws=int(st[1]))
    return KMeansResult(cent, assign, float(obj.value))


class BuiltBruteForce:
    """Host-resident brute-force index: the per-vector arrays of `BruteForceRabitqIndex` (src/brute_force.rs:202-210)."""

    def __init__(self, handle):
        self._h = handle
        self.hdr_ptr = lib().rbq_bf_built_header(handle)
        self.view_ptr = lib().rbq_bf_built_view(handle)

    @property
    def header(self):
        return self.hdr_ptr.contents

    @property
    def t_const(self):
        """Constant rescale factor of the faster config (0.0 when it was not used)."""
        return float(lib().rbq_bf_built_t_const(self._h))

    def __len__(self):
        return int(self.view_ptr.contents.n)

    def arrays(self):
        """numpy copies: bin [n][D/8] u8, ex [n][ex_len] u8, and the 8 factor arrays by name."""
        v, h = self.view_ptr.contents, self.header
        n, D = int(v.n), int(h.padded_dim)
        out = {"bin": np.ctypeslib.as_array(v.bin_codes, shape=(n, D // 8)).copy(),
               "ex": (np.ctypeslib.as_array(v.ex_codes, shape=(n, int(v.ex_len))).copy() if v.ex_len
                      else np.zeros((n, 0), np.uint8))}
        for f in BF_FACTORS:
            out[f] = np.ctypeslib.as_array(getattr(v, f), shape=(n,)).copy()
        return out

    def rotator_blob(self):
        h = self.header
        return bytes(np.ctypeslib.as_array(h.rotator_blob, shape=(int(h.rotator_len),))) if h.rotator_len else b""

    def rotate(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.header.padded_dim, np.float32)
        lib().rbq_build_rotate(self.hdr_ptr, x.ctypes.data, out.ctypes.data)
        return out

    def close(self):
        if self._h:
            lib().rbq_bf_built_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_bruteforce(data, total_bits, metric, rotator_type, seed, use_faster_config):
    """`BruteForceRabitqIndex::train` (src/brute_force.rs:214-287).  Errors in the crate's order."""
    from . import RabitqError
    from ._abi import RBQ_INVALID_CONFIG
    data = np.ascontiguousarray(data, dtype=np.float32)
    if data.ndim != 2 or data.shape[0] == 0:
        raise RabitqError(RBQ_INVALID_CONFIG, "training data must be non-empty")
    if not 1 <= int(total_bits) <= 16:
        raise RabitqError(RBQ_INVALID_CONFIG, "total_bits must be between 1 and 16")
    n, dim = data.shape
    h = C.c_void_p()
    rc = lib().rbq_build_train_bruteforce(data.ctypes.data, n, dim, int(total_bits), int(metric), int(rotator_type), int(seed),
                                          int(bool(use_faster_config)), C.byref(h))
    if rc != RBQ_OK:
        raise RabitqError(rc, "total_bits %d (ex_bits %d) is not supported: only 1, 3 and 7 total bits" % (total_bits, total_bits - 1)
                          if total_bits - 1 not in (0, 2, 6) else NOT_MULTIPLE_OF_16 if rotator_type != ROTATOR_FHT_KAC and dim % 16
                          else "train_bruteforce rejected its configuration")
    return BuiltBruteForce(h)
