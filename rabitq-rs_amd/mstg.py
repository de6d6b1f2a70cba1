"""MSTG on the GPU (include/rbq_mstg.h).  Build: steps 2 and 3 of `MstgIndex::build` (reference src/mstg/index.rs:40-110),
closure assignment with the RNG rule (`ClosureAssigner::assign`, src/mstg/closure.rs) and the posting lists of the expanded
(vector, list) pairs.  Search: `MstgIndex::search` / `batch_search` in one call (`mstg_search`): the exact ef_search nearest
centroids, dynamic_prune and the posting-list scan.

The arithmetic is the crate's on an AVX2 host; `closure_assign_cpu` (csrc/host/rbq_build.cpp) restates it on the CPU and the
device result equals it exactly; `select_lists_cpu` does the same for the search's list selection
(section 16).  Step 1, `HierarchicalClustering::cluster` (src/mstg/clustering.rs), is `hierarchical_cluster` (restated by
`hierarchical_cluster_cpu`, section 17), and `MstgIndex` strings the steps together as the crate's Python binding does.  The HNSW
over the centroids is not built: the search ranks the centroids exactly.

Persistence (include/rbq_mstg_persist.h): `save_mstg` / `load_mstg` and `MstgIndex.save` / `load` write and
read the crate's `{path}.mstg` (src/mstg/io.rs), assembled and taken apart on the GPU.  The crate's HNSW side files
(`{path}.hnsw.graph`, `{path}.hnsw.data`) are neither written nor read: a crate-written index loads here, while the crate cannot
reopen a file written here without side files of its own making."""
import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._marshal import ids_arg, owned_bytes, reader_callback, rows_arg, torch_of, writer_callback

NONE = 0xFFFFFFFF  # unused slot of a closure row


def _host_f32(a):
    if hasattr(a, "detach"):  # a torch tensor
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _shapes(data, centroids):
    from . import RabitqError
    if len(data.shape) != 2 or len(centroids.shape) != 2 or data.shape[1] != centroids.shape[1]:
        raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data [n][dim], centroids [n_lists][dim]")
    return int(data.shape[0]), int(centroids.shape[0]), int(data.shape[1])


def closure_assign_cpu(data, centroids, epsilon, max_replicas):
    """`ClosureAssigner::new(epsilon, max_replicas).assign(row, centroids)` for every row, on the CPU (OpenMP over the rows):
    (lists [n][max_replicas] u32 in the crate's Vec order with NONE in unused slots, counts [n] u32)."""
    from . import RabitqError, builder
    x, c = _host_f32(data), _host_f32(centroids)
    n, k, dim = _shapes(x, c)
    lists = np.empty((n, max(int(max_replicas), 0)), np.uint32)
    counts = np.empty(n, np.uint32)
    rc = builder.lib().rbq_build_closure_assign(c.ctypes.data, k, dim, x.ctypes.data, n, float(epsilon), int(max_replicas),
                                                lists.ctypes.data, counts.ctypes.data)
    if rc != _abi.RBQ_OK:
        raise RabitqError(rc, "closure assignment rejected its configuration")
    return lists, counts


def closure_assign(data, centroids, epsilon, max_replicas, device=None, max_chunk_rows=0):
    """The same on the GPU (rbq_mstg_closure_assign).  `data` and `centroids` are NumPy arrays (host rows are copied a chunk at a
    time) or CUDA tensors (used in place).  Returns host arrays equal to closure_assign_cpu's."""
    from .index import _check, lib
    n, k, dim = _shapes(data, centroids)
    dev = -1 if device is None else int(device)
    xp, _x = rows_arg(data)
    cp, _c = rows_arg(centroids)
    lists = np.empty((n, max(int(max_replicas), 0)), np.uint32)
    counts = np.empty(n, np.uint32)
    _check(lib().rbq_mstg_closure_assign(cp, k, dim, xp, n, float(epsilon), int(max_replicas), int(max_chunk_rows), dev,
                                         lists.ctypes.data, counts.ctypes.data))
    return lists, counts


def closure_fallbacks():
    """Rows of every closure assignment so far that were scored against every centroid (rbq_mstg_debug_closure_fallbacks)."""
    from .index import lib
    return int(lib().rbq_mstg_debug_closure_fallbacks())


def debug_closure_shortlist(data, centroids, max_replicas, device=None, max_chunk_rows=0):
    """Test hook (rbq_mstg_debug_closure_shortlist): (sl [n][256] u32, sl_n [n] u32; sl_n NONE = the row falls back)."""
    from .index import _check, lib
    n, k, dim = _shapes(data, centroids)
    dev = -1 if device is None else int(device)
    xp, _x = rows_arg(data)
    cp, _c = rows_arg(centroids)
    sl = np.empty((n, 256), np.uint32)
    sl_n = np.empty(n, np.uint32)
    _check(lib().rbq_mstg_debug_closure_shortlist(cp, k, dim, xp, n, int(max_replicas), int(max_chunk_rows), dev, sl.ctypes.data,
                                                  sl_n.ctypes.data))
    return sl, sl_n


def expand_pairs(lists, counts):
    """(pair_vec, pair_list) of a closure, sorted by (list, vector): the order the posting lists hold them in."""
    lists, counts = np.asarray(lists), np.asarray(counts)
    keep = np.arange(lists.shape[1])[None, :] < counts[:, None]
    vec = np.broadcast_to(np.arange(lists.shape[0], dtype=np.int64)[:, None], lists.shape)[keep]
    lst = lists[keep].astype(np.int64)
    order = np.lexsort((vec, lst))
    return vec[order], lst[order].astype(np.uint32)


def build_postings_on_device(data, centroids, total_bits, metric, closure_epsilon=0.15, max_replicas=8, faster_config=False,
                             device=None, max_chunk_rows=0):
    """MstgIndex::build steps 2 and 3 on the GPU (rbq_mstg_build_device): an IvfRabitqIndex handle with rotator NoRotation that
    `posting_scan` serves; list c holds its vectors in ascending index, ids are the row indices.  The header, and t_const for
    `faster_config` (what PostingList::quantize_vectors derives with seed 42), come from the CPU builder over one row: both
    depend on (dim, bits, seed) only, and the copy of the header that is handed over names all the lists."""
    from . import RabitqError, RotatorType, builder
    from .index import IvfRabitqIndex, _check, _rescale, lib
    n, k, dim = _shapes(data, centroids)
    dev = -1 if device is None else int(device)
    xp, _x = rows_arg(data)
    cent = _host_f32(centroids)
    if n == 0 or k == 0:
        raise RabitqError(_abi.RBQ_INVALID_CONFIG, "data and centroids must be non-empty")
    small = builder.train_with_clusters(cent[:1], cent[:1], np.zeros(1, np.uint32), total_bits, metric, RotatorType.NoRotation, 42, True)
    try:
        hdr = _abi.Header.from_buffer_copy(small.header)  # (NoRotation: no rotator blob to keep alive)
        t_const = small.t_const
    finally:
        small.close()
    hdr.n_lists, hdr.n_vectors = k, 0
    mode, t = _rescale("const" if faster_config else "optimal", t_const if faster_config else None)
    h = C.c_void_p()
    _check(lib().rbq_mstg_build_device(C.byref(hdr), cent.ctypes.data, xp, n, float(closure_epsilon), int(max_replicas), mode, t,
                                       int(max_chunk_rows), dev, C.byref(h)))
    return IvfRabitqIndex(h)


def append_postings(handle, data, first_id=None, closure_epsilon=0.15, max_replicas=8, max_chunk_rows=0, return_lists=False):
    """FAISS-style add on an MSTG handle (rbq_mstg_append): a NEW handle that holds `handle`'s slots and those of the rows of
    `data` [count][dim] (a NumPy array, copied a chunk at a time, or a CUDA tensor, used in place), with ids first_id ..
    (None: handle.id_bound()).  Every row joins the lists its closure against the handle's own centroids names and is encoded
    with the rescale mode the handle remembers; the result equals build_postings_on_device over the old and the new rows with
    the same centroids, array for array.  `handle` stays valid; the caller closes it.  With `return_lists`, also (lists
    [count][max_replicas], counts [count]) as closure_assign returns them: NumPy u32 arrays for NumPy data, int32 tensors (bit
    patterns) on the data's device for a CUDA tensor."""
    from . import RabitqError
    from .index import IvfRabitqIndex, _check, lib
    if len(data.shape) != 2 or int(data.shape[1]) != int(handle.dim):
        raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data must be [count][%d]" % int(handle.dim))
    count, M = int(data.shape[0]), int(max_replicas)
    xp, x = rows_arg(data)
    on_dev = not isinstance(x, np.ndarray)
    lists = counts = lp = cp = None
    if return_lists:
        if on_dev:
            import torch
            lists = torch.empty((count, max(M, 0)), dtype=torch.int32, device=x.device)
            counts = torch.empty(count, dtype=torch.int32, device=x.device)
            lp, cp = C.c_void_p(lists.data_ptr()), C.c_void_p(counts.data_ptr())
        else:
            lists, counts = np.empty((count, max(M, 0)), np.uint32), np.empty(count, np.uint32)
            lp, cp = C.c_void_p(lists.ctypes.data), C.c_void_p(counts.ctypes.data)
    h = C.c_void_p()
    _check(lib().rbq_mstg_append(handle._h, xp, count, handle.id_bound() if first_id is None else int(first_id),
                                 float(closure_epsilon), M, int(max_chunk_rows), lp, cp, C.byref(h)))
    new = IvfRabitqIndex(h)
    return (new, lists, counts) if return_lists else new


def remove_postings(handle, ids):
    """FAISS-style remove_ids on an MSTG handle (rbq_mstg_remove_ids): (a NEW handle without the slots whose id is in `ids`,
    the number of slots removed — a vector held by three lists counts three).  `ids` is a NumPy u64 array (or anything that
    converts to one) or a CUDA int64 / uint64 tensor; any order, repeats allowed, ids that are not stored ignored.  The result
    equals build_postings_on_device over the rows that stay, with their original ids.  `handle` stays valid."""
    from .index import IvfRabitqIndex, _check, lib
    n, p, _ids = ids_arg(ids)  # (_ids owns what p names)
    h, removed = C.c_void_p(), C.c_uint64()
    _check(lib().rbq_mstg_remove_ids(handle._h, p if n else None, n, C.byref(removed), C.byref(h)))
    return IvfRabitqIndex(h), int(removed.value)


def append_passes():
    """Encode passes of every append_postings so far (rbq_debug_mstg_append_passes)."""
    from .index import lib
    return int(lib().rbq_debug_mstg_append_passes())


@dataclass(frozen=True)
class MstgSearchParams:
    """The crate's SearchParams of an MSTG index (src/mstg/config.rs): how many centroids are ranked, and dynamic_prune's epsilon."""
    ef_search: int = 150
    pruning_epsilon: float = 0.6

    @staticmethod
    def balanced():
        return MstgSearchParams(150, 0.6)

    @staticmethod
    def high_recall():
        return MstgSearchParams(300, 0.8)

    @staticmethod
    def low_latency():
        return MstgSearchParams(50, 0.4)


def select_lists_cpu(queries, centroids, ef_search, pruning_epsilon):
    """The list selection of `mstg_search` on the CPU (rbq_build_mstg_select_lists, OpenMP over the queries): (lists
    [nq][min(ef_search, n_lists)] u32 in scan order with NONE in unused slots, counts [nq] u32)."""
    from . import RabitqError, builder
    q, c = _host_f32(queries), _host_f32(centroids)
    nq, k, dim = _shapes(q, c)
    ef = min(max(int(ef_search), 0), k)
    lists = np.empty((nq, ef), np.uint32)
    counts = np.empty(nq, np.uint32)
    rc = builder.lib().rbq_build_mstg_select_lists(c.ctypes.data, k, dim, q.ctypes.data, nq, int(ef_search), float(pruning_epsilon),
                                                   lists.ctypes.data, counts.ctypes.data)
    if rc != _abi.RBQ_OK:
        raise RabitqError(rc, "list selection rejected its configuration")
    return lists, counts


def search_fallbacks():
    """Queries of every MSTG search so far that were scored against every centroid (rbq_mstg_debug_search_fallbacks)."""
    from .index import lib
    return int(lib().rbq_mstg_debug_search_fallbacks())


REFINE_POOL_MAX = _abi.MSTG_REFINE_POOL_MAX


@contextlib.contextmanager
def _mstg_rerank_for_call(index, exact):
    """Context of one refined call: with `exact` the handle's option "mstg_rerank" is set to 1 where it is not (read back from the
    handle) and the handle's value put back afterwards, error or not.  exact=False makes no option call: a handle whose option the
    caller set by hand keeps serving as it was told."""
    if not exact:
        yield
        return
    v = C.c_int32(-1)
    from .index import _check, lib
    _check(lib().rbq_debug_copy_index(index._h, b"mstg_rerank", C.byref(v), 4))
    if v.value == 1:
        yield
        return
    index.set_option("mstg_rerank", 1)
    try:
        yield
    finally:
        index.set_option("mstg_rerank", 0)


def mstg_search(index, queries, top_k, ef_search=150, pruning_epsilon=0.6, return_lists=False, refine_pool=None, dtype=None, exact=False):
    """`MstgIndex::batch_search` on an MSTG handle (rotator NoRotation, e.g. from build_postings_on_device) in one call:
    (ids [nq][top_k] u64, distances [nq][top_k] f32 ascending, counts [nq] u32), plus (lists, list_counts) of the selected
    posting lists in scan order with `return_lists`.  NumPy queries take rbq_mstg_search_batch and return arrays; a CUDA tensor
    takes rbq_mstg_search_batch_device on the current stream, without synchronising, and returns tensors (ids as int64 bit
    patterns, lists as int32 bit patterns: torch has no unsigned 64 / 32-bit arithmetic).

    `refine_pool=None` is the crate's search: 1-bit estimates, and an id may come back once per list that holds it.  An int takes
    rbq_mstg_search_refined_batch*: the max(refine_pool, top_k) best binary candidates are re-scored with the stored ex codes,
    reduced to one entry per id and the top_k nearest returned (at most REFINE_POOL_MAX candidates).

    `exact=True` (needs an int `refine_pool`, and raw vectors attached to the handle with set_rerank_vectors): the pool is reduced
    to one entry per id and every distinct id is scored exactly against its raw row instead of the ex codes (option "mstg_rerank",
    set for the call and put back afterwards).  Distances are the canonical l2_distance_sqr, or minus the
    canonical dot product.  Without vectors attached, or with the handle's "rerank" off, the library refuses the call.

    Queries of 16 bits (a numpy.float16 array, a torch.half / torch.bfloat16 tensor, a numpy.uint16 array of bit patterns with
    dtype="f16" | "bf16") are read as they are: the handle's option "query_dtype" is set for the call and put back afterwards."""
    from . import _marshal
    from .index import _check, lib
    top_k, ef_search = int(top_k), int(ef_search)
    L = lib()
    if exact and refine_pool is None:
        raise ValueError("exact=True needs refine_pool: the exact rerank scores the pool of the refined search")
    if refine_pool is None:
        host_fn, dev_fn, extra = L.rbq_mstg_search_batch, L.rbq_mstg_search_batch_device, ()
    else:
        host_fn, dev_fn, extra = L.rbq_mstg_search_refined_batch, L.rbq_mstg_search_refined_batch_device, (int(refine_pool),)
    ef = min(max(ef_search, 0), index.cluster_count())
    q, code = _marshal.query_arg(queries, dtype)
    torch = torch_of(q)
    if torch is not None and q.is_cuda:
        nq, qd = q.shape
        with torch.cuda.device(q.device):
            ids = torch.empty((nq, top_k), dtype=torch.int64, device=q.device)
            sc = torch.empty((nq, top_k), dtype=torch.float32, device=q.device)
            cnt = torch.empty(nq, dtype=torch.int32, device=q.device)
            li = torch.empty((nq, ef), dtype=torch.int32, device=q.device) if return_lists else None
            lc = torch.empty(nq, dtype=torch.int32, device=q.device) if return_lists else None
            stream = torch.cuda.current_stream().cuda_stream
            with index._query_dtype_for_call(code), _mstg_rerank_for_call(index, exact):
                rc = dev_fn(index._h, q.data_ptr(), nq, qd, top_k, ef_search, float(pruning_epsilon), *extra,
                            ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(),
                            li.data_ptr() if return_lists else None, lc.data_ptr() if return_lists else None,
                            C.c_void_p(stream))
            _check(rc)
        return (ids, sc, cnt, li, lc) if return_lists else (ids, sc, cnt)
    nq, qd = q.shape
    ids = np.empty((nq, top_k), np.uint64)
    sc = np.empty((nq, top_k), np.float32)
    cnt = np.zeros(nq, np.uint32)
    li = np.empty((nq, ef), np.uint32) if return_lists else None
    lc = np.empty(nq, np.uint32) if return_lists else None
    with index._query_dtype_for_call(code), _mstg_rerank_for_call(index, exact):
        rc = host_fn(index._h, _marshal.data_ptr(q), nq, qd, top_k, ef_search, float(pruning_epsilon), *extra, ids.ctypes.data,
                     sc.ctypes.data, cnt.ctypes.data, li.ctypes.data if return_lists else None,
                     lc.ctypes.data if return_lists else None)
    _check(rc)
    return (ids, sc, cnt, li, lc) if return_lists else (ids, sc, cnt)


def _config_struct(config):
    cfg = config if isinstance(config, _abi.MstgConfig) else _abi.MstgConfig.from_dict(config)
    return cfg


def save_mstg(index, config, dest):
    """Write the `.mstg` stream of an MSTG handle (rbq_mstg_save_stream).  `config` is a dict of the thirteen MstgConfig fields
    (_abi.MSTG_CONFIG_FIELDS; metric 0 / 1, centroid_precision 0..3) or an _abi.MstgConfig; `dest` a path (the file is created or
    truncated; the crate's name is `{base}.mstg`) or anything with .write(bytes).  Chunks arrive as the device finishes them; a
    writer exception stops the save and is re-raised."""
    from . import RabitqError
    from .index import _check, lib
    cfg = _config_struct(config)
    if isinstance(dest, (str, bytes)) or hasattr(dest, "__fspath__"):
        try:
            f = open(dest, "wb")
        except OSError as e:
            raise RabitqError(_abi.RBQ_IO, str(e))
        with f:
            return save_mstg(index, cfg, f)
    fn, err = writer_callback(dest)
    rc = lib().rbq_mstg_save_stream(index._h, C.byref(cfg), fn, None)
    if err:
        raise err[0]
    _check(rc)


def save_mstg_bytes(index, config):
    """The whole `.mstg` stream as bytes (rbq_mstg_save)."""
    from .index import _check, lib
    cfg = _config_struct(config)
    return owned_bytes(lambda p, n: _check(lib().rbq_mstg_save(index._h, C.byref(cfg), p, n)), lib().rbq_persist_free_bytes)


def load_mstg(src, device=None):
    """(handle, config dict) of a `.mstg` stream: `src` is bytes (rbq_mstg_load), or a path or a seekable binary file, read
    through rbq_mstg_load_stream (the framing first, then the records span by span: host memory stays two spans)."""
    from . import RabitqError
    from .index import IvfRabitqIndex, _check, lib
    dev = -1 if device is None else int(device)
    cfg, h = _abi.MstgConfig(), C.c_void_p()
    if isinstance(src, (bytes, bytearray, memoryview)):
        data = bytes(src)
        _check(lib().rbq_mstg_load(data, len(data), dev, C.byref(cfg), C.byref(h)))
        return IvfRabitqIndex(h), cfg.to_dict()
    if isinstance(src, str) or hasattr(src, "__fspath__"):
        try:
            f = open(src, "rb")
        except OSError as e:
            raise RabitqError(_abi.RBQ_IO, str(e))
        with f:
            return load_mstg(f, device)
    total = src.seek(0, 2)
    fn, err = reader_callback(src, 0)
    rc = lib().rbq_mstg_load_stream(fn, None, total, dev, C.byref(cfg), C.byref(h))
    if err:
        raise err[0]
    _check(rc)
    return IvfRabitqIndex(h), cfg.to_dict()


def memory_usage(index):
    """Device bytes an MSTG handle holds on its first device (rbq_mstg_memory_usage)."""
    from .index import lib
    return int(lib().rbq_mstg_memory_usage(index._h))


def _hc_args(max_posting_size, branching_factor, max_iterations):
    from . import RabitqError
    v = [int(max_posting_size), int(branching_factor), int(max_iterations)]
    if min(v) < 0:
        raise RabitqError(_abi.RBQ_INVALID_CONFIG, "max_posting_size, branching_factor and max_iterations must not be negative")
    return v


def hierarchical_cluster_cpu(data, max_posting_size, branching_factor=10, balance_weight=1.0, max_iterations=100, device=None,
                             host_below=None):
    """`HierarchicalClustering{max_posting_size, branching_factor, balance_weight, max_iterations}.cluster(data)` on the CPU
    (rbq_build_hcluster): (centroids [count][dim] f32, offsets [count + 1] u64, members [n] u32, stats) with the final clusters
    in the crate's pop order and every cluster's rows in its own order.  `device` and `host_below` are accepted and ignored, so
    that both functions take the same arguments."""
    from . import RabitqError, builder
    x = _host_f32(data)
    if len(x.shape) != 2:
        raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data [n][dim]")
    n, dim = int(x.shape[0]), int(x.shape[1])
    mps, k, it = _hc_args(max_posting_size, branching_factor, max_iterations)
    h, detail = C.c_void_p(), C.c_char_p()
    L = builder.lib()
    rc = L.rbq_build_hcluster(x.ctypes.data if n and dim else None, n, dim, mps, k, float(balance_weight), it, C.byref(h), C.byref(detail))
    if rc != _abi.RBQ_OK:
        raise RabitqError(rc, (detail.value or b"").decode())
    return builder.take_hclustered(L, h, n, dim)


def hierarchical_cluster(data, max_posting_size, branching_factor=10, balance_weight=1.0, max_iterations=100, device=None,
                         host_below=None):
    """The same on the GPU (rbq_mstg_cluster_device), bit for bit.  `data` is a NumPy array (uploaded once) or a CUDA tensor (used
    in place).  A cluster of at most `host_below` rows is handed to the host with its whole subtree (small splits are bound by
    launch latency); the result does not depend on it.  None takes the library's default, 0 never hands over."""
    from . import RabitqError, builder
    from .index import _check, lib
    if len(data.shape) != 2:
        raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data [n][dim]")
    n, dim = int(data.shape[0]), int(data.shape[1])
    mps, k, it = _hc_args(max_posting_size, branching_factor, max_iterations)
    dev = -1 if device is None else int(device)
    xp, _x = rows_arg(data)
    hb = HOST_BELOW_DEFAULT if host_below is None else int(host_below)
    h = C.c_void_p()
    L = lib()
    _check(L.rbq_mstg_cluster_device(xp if n and dim else None, n, dim, mps, k, float(balance_weight), it, hb, dev, C.byref(h)))
    return builder.take_hclustered(L, h, n, dim)


HOST_BELOW_DEFAULT = 0xFFFFFFFFFFFFFFFF  # RBQ_MSTG_HOST_BELOW_DEFAULT: let the library choose

_KEEP = object()  # set_query_arguments: "leave refine_pool as it is" (None is a value of its own)
_METRICS = {"euclidean": 0, "l2": 0, "angular": 1, "ip": 1, "inner_product": 1}


class MstgIndex:
    """The crate's `PyMstgIndex` (src/python_bindings.rs) on the GPU: the same constructor arguments and defaults, `fit`,
    `set_query_arguments`, `query`, `batch_query`.  `fit` runs hierarchical_cluster and build_postings_on_device, so the
    dimension must be a multiple of 16; queries go through mstg_search.

    `hnsw_m`, `hnsw_ef_construction` and `centroid_precision` are accepted and recorded, and unused: the crate needs them for the
    HNSW over its (quantised) centroids, while this library ranks the full-precision centroids exactly (rbq_mstg.h, "the
    selection").  `save(path)` / `load(path)` write and read the crate's `{path}.mstg` on the GPU; the crate's HNSW side files are
    neither written nor read, so the crate cannot reopen a file saved here.  `get_memory_usage()` is the
    device footprint in bytes.  As in the crate, results are [count][2] f32 arrays of (id, distance), which
    hold ids exactly only below 2^24; `mstg_search(index.handle, ...)` returns u64 ids."""

    def __init__(self, dimension, metric="euclidean", max_posting_size=16, branching_factor=10, balance_weight=1.0,
                 closure_epsilon=0.15, max_replicas=8, rabitq_bits=7, faster_config=True, hnsw_m=32, hnsw_ef_construction=400,
                 centroid_precision="bf16", default_ef_search=150, pruning_epsilon=0.6, device=None, max_iterations=100,
                 host_below=None):
        if metric not in _METRICS:
            raise ValueError(f"Invalid metric: {metric}. Use 'euclidean' or 'angular'")
        if centroid_precision not in ("fp32", "bf16", "fp16", "int8"):
            raise ValueError(f"Invalid precision: {centroid_precision}. Use 'fp32', 'bf16', 'fp16', or 'int8'")
        self.dimension, self.metric = int(dimension), _METRICS[metric]
        self.max_posting_size, self.branching_factor, self.balance_weight = int(max_posting_size), int(branching_factor), float(balance_weight)
        self.closure_epsilon, self.max_replicas = float(closure_epsilon), int(max_replicas)
        self.rabitq_bits, self.faster_config = int(rabitq_bits), bool(faster_config)
        self.hnsw_m, self.hnsw_ef_construction, self.centroid_precision = int(hnsw_m), int(hnsw_ef_construction), centroid_precision
        self.default_ef_search, self.pruning_epsilon = int(default_ef_search), float(pruning_epsilon)
        self.device, self.max_iterations, self.host_below = device, int(max_iterations), host_below
        self.handle, self.centroids, self.cluster_stats, self._n = None, None, None, 0
        self.refine_pool = None  # the crate's search; set_query_arguments(refine_pool=...) switches to the refined one
        self.exact = False       # set_query_arguments(exact=True): the refined search scores its pool against the attached raw vectors

    def fit(self, data):
        if len(data.shape) != 2:
            raise ValueError("Data must be 2D array (N x D)")
        if data.shape[1] != self.dimension:
            raise ValueError(f"Data dimension {data.shape[1]} does not match expected {self.dimension}")
        cent, _off, _mem, st = hierarchical_cluster(data, self.max_posting_size, self.branching_factor, self.balance_weight,
                                                    self.max_iterations, self.device, self.host_below)
        self.handle = build_postings_on_device(data, cent, self.rabitq_bits, self.metric, self.closure_epsilon, self.max_replicas,
                                               self.faster_config, self.device)
        self.centroids, self.cluster_stats, self._n = cent, st, int(data.shape[0])
        return self

    def set_rerank_vectors(self, vectors=None, device_ptr=None, n=0, dtype=None):
        """Attach raw vectors to the handle (IvfRabitqIndex.set_rerank_vectors: a host array [n][dim] or `device_ptr` + n, as
        "f32", "f16" or "bf16"; None detaches): row i is the vector of id i.  Only queries with `exact=True` read them.  `add` and
        `remove_ids` swap the handle, and the new one has no vectors attached: attach rows that cover the new ids again."""
        self._built().set_rerank_vectors(vectors, device_ptr, n, dtype=dtype)

    def set_query_arguments(self, ef_search=None, pruning_epsilon=None, refine_pool=_KEEP, exact=_KEEP):
        """`refine_pool`: None = the crate's search (the default); an int = the refined search of `mstg_search` over a pool of that
        many binary candidates (ex-code distances, every id once).  Left out, it keeps its value.
        `exact`: True = the refined search scores its pool exactly against the vectors of set_rerank_vectors (mstg_search's
        `exact`; needs an int refine_pool).  Left out, it keeps its value."""
        if ef_search is not None:
            self.default_ef_search = int(ef_search)
        if pruning_epsilon is not None:
            self.pruning_epsilon = float(pruning_epsilon)
        if refine_pool is not _KEEP:
            self.refine_pool = None if refine_pool is None else int(refine_pool)
        if exact is not _KEEP:
            self.exact = bool(exact)

    def _built(self):
        if self.handle is None:
            raise RuntimeError("Index not built yet. Call fit() first.")
        return self.handle

    def batch_query(self, queries, k, dtype=None):
        """`queries` [N][D]: f32, or 16-bit rows read as they are (mstg_search's `queries` and `dtype`; host arrays or tensors)."""
        from . import _marshal
        h = self._built()
        q, dtype = _marshal.query_arg(queries, dtype)
        if _marshal.torch_of(q) is not None and q.is_cuda:
            raise ValueError("Queries must be on the host (mstg_search takes CUDA tensors)")
        if len(q.shape) != 2:
            raise ValueError("Queries must be 2D array (N x D)")
        if q.shape[1] != self.dimension:
            raise ValueError(f"Query dimension {q.shape[1]} does not match expected {self.dimension}")
        ids, dist, cnt = mstg_search(h, q, k, self.default_ef_search, self.pruning_epsilon, refine_pool=self.refine_pool, dtype=dtype,
                                     exact=self.exact)
        return [np.stack([ids[i, :cnt[i]].astype(np.float32), dist[i, :cnt[i]]], axis=1) for i in range(q.shape[0])]

    def query(self, query, k, dtype=None):
        from . import _marshal
        q, dtype = _marshal.query_arg(query, dtype)
        if q.ndim != 1 or q.shape[0] != self.dimension:
            raise ValueError(f"Query dimension {q.shape[-1] if q.ndim else 0} does not match expected {self.dimension}")
        return self.batch_query(q[None, :], k, dtype)[0]

    def config(self):
        """The crate's MstgConfig of this index (what `save` writes)."""
        return dict(max_posting_size=self.max_posting_size, branching_factor=self.branching_factor, balance_weight=self.balance_weight,
                    closure_epsilon=self.closure_epsilon, max_replicas=self.max_replicas, rabitq_bits=self.rabitq_bits,
                    faster_config=self.faster_config, metric=self.metric, hnsw_m=self.hnsw_m,
                    hnsw_ef_construction=self.hnsw_ef_construction,
                    centroid_precision=_abi.MSTG_PRECISIONS.index(self.centroid_precision),
                    default_ef_search=self.default_ef_search, pruning_epsilon=self.pruning_epsilon)

    def save(self, path):
        """`MstgIndex::save_to_path`'s main file: writes `{path}.mstg` (only: see the class docstring on the HNSW side files)."""
        save_mstg(self._built(), self.config(), str(path) + ".mstg")

    @staticmethod
    def load(path, device=None):
        """Reads `{path}.mstg` onto `device`: every constructor field comes from the file's config, the centroids from the
        posting lists, and len() is 1 + the largest vector id."""
        handle, cfg = load_mstg(str(path) + ".mstg", device)
        self = MstgIndex(int(handle.dim), "euclidean" if cfg["metric"] == 0 else "angular", cfg["max_posting_size"], cfg["branching_factor"],
                         cfg["balance_weight"], cfg["closure_epsilon"], cfg["max_replicas"], cfg["rabitq_bits"], cfg["faster_config"],
                         cfg["hnsw_m"], cfg["hnsw_ef_construction"], _abi.MSTG_PRECISIONS[cfg["centroid_precision"]],
                         cfg["default_ef_search"], cfg["pruning_epsilon"], device)
        k, D = int(handle.cluster_count()), int(handle.dim)
        self.handle = handle
        self.centroids = handle.debug_copy_index("centroids", np.empty((k, D), np.float32))
        ln = handle.debug_copy_index("list_n", np.empty(k, np.uint32))
        ids = handle.debug_copy_index("ids", np.empty(int(((ln.astype(np.int64) + 31) // 32).sum()) * 32, np.uint64))
        real = ids[ids != np.uint64(0xFFFFFFFFFFFFFFFF)]
        self._n = int(real.max()) + 1 if real.size else 0
        return self

    def id_bound(self):
        """1 + the largest stored id (rbq_index_id_bound)."""
        return self._built().id_bound()

    def add(self, data):
        """FAISS-style add (append_postings with this object's closure_epsilon and max_replicas): the rows of `data` join the
        posting lists with the ids id_bound() ..; nothing is re-clustered, the centroids stay.  The handle is swapped for the
        grown one and the old one closed.  Returns the first new id.
        The new handle has no raw vectors attached: a query with exact=True is refused by the library (RabitqError) until
        set_rerank_vectors attaches rows that cover the new ids too.  Nothing is re-attached silently."""
        h = self._built()
        if len(data.shape) != 2:
            raise ValueError("Data must be 2D array (N x D)")
        if data.shape[1] != self.dimension:
            raise ValueError(f"Data dimension {data.shape[1]} does not match expected {self.dimension}")
        first = h.id_bound()
        self.handle = append_postings(h, data, first, self.closure_epsilon, self.max_replicas)
        h.close()
        self._n = self.handle.id_bound()
        return first

    def remove_ids(self, ids):
        """FAISS-style remove_ids (remove_postings): every slot whose id is in `ids` leaves its list.  The handle is swapped for
        the shrunk one and the old one closed; len() becomes 1 + the largest id that stays.  Returns the number of slots removed
        (a vector counts once per list that held it).
        The new handle has no raw vectors attached: a query with exact=True is refused by the library (RabitqError) until
        set_rerank_vectors attaches them again.  Nothing is re-attached silently."""
        h = self._built()
        self.handle, removed = remove_postings(h, ids)
        h.close()
        self._n = self.handle.id_bound()
        return removed

    def get_memory_usage(self):
        """Device bytes held by the index (the crate's get_memory_usage reports its host footprint)."""
        return memory_usage(self._built())

    def __len__(self):
        return self._n

    def __repr__(self):
        built = f"{self._n} vectors, {len(self.centroids)} posting lists" if self.handle is not None else "not built"
        return (f"MstgIndex(dimension={self.dimension}, metric={'l2' if self.metric == 0 else 'ip'}, "
                f"max_posting_size={self.max_posting_size}, rabitq_bits={self.rabitq_bits}, {built})")
