"""The Python mirror of the C ABI, as data: the constants and data-contract structs of include/*.h, and one prototype table per
shared library: name -> (restype, [argtypes]) of every entry point of librbq.so (include/*.h, grouped by header) and of
librbq_build.so (csrc/host/rbq_build.h).  `bind` applies a table to a loaded library; index.lib() and builder.lib() do nothing
else.  A new entry point is declared for Python by one line in its header's group.  tests/test_abi_prototypes.py holds every
line, struct field and constant here to the headers."""
import ctypes as C

RBQ_OK, RBQ_DIMENSION_MISMATCH, RBQ_INVALID_CONFIG, RBQ_EMPTY_INDEX, RBQ_IO, \
    RBQ_INVALID_PERSISTENCE, RBQ_DEVICE = range(7)
METRIC_L2, METRIC_IP = 0, 1
ROTATOR_MATRIX, ROTATOR_FHT_KAC, ROTATOR_NONE = 0, 1, 2
# numeric variants (RBQ_NUMERIC_*): which build of the reference the scores reproduce bit for bit
NUMERIC_NATIVE_AVX512, NUMERIC_NATIVE_AVX2, NUMERIC_PORTABLE = 0, 1, 2
NUMERIC_VARIANTS = {"native_avx512": NUMERIC_NATIVE_AVX512, "native_avx2": NUMERIC_NATIVE_AVX2, "portable": NUMERIC_PORTABLE}
# rescale modes of the device encoder (RBQ_RESCALE_*): RabitqConfig::faster / RabitqConfig::new
RESCALE_CONST, RESCALE_OPTIMAL = 0, 1
RESCALE_MODES = {"const": RESCALE_CONST, "optimal": RESCALE_OPTIMAL}
# element types of the rerank's raw rows (RBQ_RAW_*): the values of the option "rerank_raw_dtype"
RAW_F32, RAW_F16, RAW_BF16 = 0, 1, 2
RAW_DTYPES = {"f32": RAW_F32, "f16": RAW_F16, "bf16": RAW_BF16}
BATCH = 32
# rbq_kmeans_device (include/rbq_kmeans.h): the config fields in ABI order and the stats slots
KMEANS_CONFIG_FIELDS = ("niter", "nredo", "seed", "spherical", "max_points_per_centroid", "decode_block_size")
KMEANS_STATS = ("shortlist_fallbacks", "empty_reseeded", "rng_draws", "max_shortlist")


class Header(C.Structure):
    _fields_ = [("dim", C.c_uint32), ("padded_dim", C.c_uint32),
                ("metric", C.c_uint8), ("rotator", C.c_uint8), ("ex_bits", C.c_uint8), ("reserved", C.c_uint8),
                ("n_vectors", C.c_uint64), ("n_lists", C.c_uint64),
                ("rotator_blob", C.POINTER(C.c_uint8)), ("rotator_len", C.c_uint64)]


class ListView(C.Structure):
    _fields_ = [("centroid", C.POINTER(C.c_float)), ("n", C.c_uint64), ("ids", C.POINTER(C.c_uint64)),
                ("batch_data", C.POINTER(C.c_uint8)), ("batch_len", C.c_uint64),
                ("ex_codes", C.POINTER(C.c_uint8)), ("f_add_ex", C.POINTER(C.c_float)),
                ("f_rescale_ex", C.POINTER(C.c_float))]


class Diag(C.Structure):
    _fields_ = [("estimated", C.c_uint64), ("skipped_by_lower_bound", C.c_uint64),
                ("extended_evaluations", C.c_uint64)]


BF_FACTORS = ("delta", "vl", "f_add", "f_rescale", "f_error", "residual_norm", "f_add_ex", "f_rescale_ex")


class BfView(C.Structure):
    """rbq_bf_view: the per-vector arrays of a brute-force index."""
    _fields_ = [("n", C.c_uint64), ("bin_codes", C.POINTER(C.c_uint8)), ("ex_codes", C.POINTER(C.c_uint8)),
                ("ex_len", C.c_uint64)] + [(f, C.POINTER(C.c_float)) for f in BF_FACTORS]


MSTG_CONFIG_FIELDS = ("max_posting_size", "branching_factor", "balance_weight", "closure_epsilon", "max_replicas", "rabitq_bits",
                      "faster_config", "metric", "hnsw_m", "hnsw_ef_construction", "centroid_precision", "default_ef_search",
                      "pruning_epsilon")
MSTG_PRECISIONS = ("fp32", "bf16", "fp16", "int8")  # ScalarPrecision's variant order (src/mstg/config.rs)
MSTG_REFINE_POOL_MAX = 4096  # RBQ_MSTG_REFINE_POOL_MAX: the largest max(refine_pool, top_k) of the refined MSTG search


class MstgConfig(C.Structure):
    """rbq_mstg_config (include/rbq_mstg_persist.h): the crate's MstgConfig, field for field."""
    _fields_ = [("max_posting_size", C.c_uint64), ("branching_factor", C.c_uint64), ("balance_weight", C.c_float),
                ("closure_epsilon", C.c_float), ("max_replicas", C.c_uint64), ("rabitq_bits", C.c_uint64),
                ("faster_config", C.c_uint8), ("metric", C.c_uint32), ("hnsw_m", C.c_uint64),
                ("hnsw_ef_construction", C.c_uint64), ("centroid_precision", C.c_uint32), ("default_ef_search", C.c_uint64),
                ("pruning_epsilon", C.c_float)]

    @classmethod
    def from_dict(cls, d):
        return cls(**{f: (int(bool(d[f])) if f == "faster_config" else d[f]) for f in MSTG_CONFIG_FIELDS})

    def to_dict(self):
        d = {f: getattr(self, f) for f in MSTG_CONFIG_FIELDS}
        d["faster_config"] = bool(d["faster_config"])
        return d


# rbq_write_fn: int (*)(void* user, const void* bytes, uint64_t len)
WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)
# rbq_read_fn: int (*)(void* user, uint64_t offset, void* dst, uint64_t len)
READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)

# ---- the prototype tables: name -> (restype, [argtypes]), argument for argument as the header declares them -------------------
_INT, _U8, _U32, _U64, _SZ, _F32, _F64, _VP, _STR = (C.c_int, C.c_uint8, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float, C.c_double,
                                                     C.c_void_p, C.c_char_p)
_OUT = C.POINTER(_VP)                   # rbq_index** and the like: a handle comes back through it
_PU64 = C.POINTER(_U64)
_BYTES = C.POINTER(C.POINTER(_U8))      # uint8_t** of the save calls: a buffer the library allocates

# the accessors of an rbq_hclustered handle: include/rbq_mstg.h and rbq_build.h both declare them, both libraries export them
HCLUSTERED = {
    "rbq_hclustered_count": (_U64, [_VP]),
    "rbq_hclustered_centroids": (C.POINTER(_F32), [_VP]),
    "rbq_hclustered_offsets": (_PU64, [_VP]),
    "rbq_hclustered_members": (C.POINTER(_U32), [_VP]),
    "rbq_hclustered_stats": (_PU64, [_VP]),
    "rbq_hclustered_free": (None, [_VP]),
}

LIBRBQ_BY_HEADER = {
    # include/rbq.h
    "rbq.h": {
        "rbq_index_create": (_INT, [_VP, _VP, _INT, _VP, _OUT]),
        "rbq_index_load_rbq1": (_INT, [_VP, _SZ, _INT, _VP, _OUT]),
        "rbq_index_build_device": (_INT, [_VP, _VP, _VP, _VP, _U64, _F32, _INT, _VP]),
        "rbq_index_build_device_ex": (_INT, [_VP, _VP, _VP, _VP, _U64, _INT, _F32, _INT, _VP]),
        "rbq_build_stream_begin": (_INT, [_VP, _VP, _VP, _F32, _INT, _OUT]),
        "rbq_build_stream_begin_ex": (_INT, [_VP, _VP, _VP, _INT, _F32, _INT, _OUT]),
        "rbq_build_stream_push": (_INT, [_VP, _VP, _VP, _U64, _U64]),
        "rbq_build_stream_finish": (_INT, [_VP, _INT, _VP, _OUT]),
        "rbq_build_stream_abort": (None, [_VP]),
        "rbq_index_destroy": (None, [_VP]),
        "rbq_index_len": (_U64, [_VP]),
        "rbq_index_cluster_count": (_U64, [_VP]),
        "rbq_index_dim": (_U32, [_VP]),
        "rbq_index_padded_dim": (_U32, [_VP]),
        "rbq_index_device_count": (_U32, [_VP]),
        "rbq_search_batch": (_INT, [_VP, _VP, _U64, _U32, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP]),
        "rbq_posting_scan_batch": (_INT, [_VP, _VP, _U64, _U32, _U32, _VP, _VP, _U32, _VP, _VP, _VP]),
        "rbq_search_batch_device": (_INT, [_VP, _VP, _U64, _U32, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP, _VP]),
        "rbq_release_stream": (_INT, [_VP, _VP]),
        "rbq_index_fetch_embeddings": (_INT, [_VP, _VP, _U64, _VP, _VP]),
        "rbq_index_fetch_embeddings_device": (_INT, [_VP, _VP, _U64, _VP, _VP, _VP]),
        "rbq_host_alloc": (_VP, [_SZ]),
        "rbq_host_free": (None, [_VP]),
        "rbq_index_set_rerank_vectors": (_INT, [_VP, _VP, _U64]),
        "rbq_index_set_numeric_variant": (_INT, [_VP, _INT]),
        "rbq_index_numeric_variant": (_INT, [_VP]),
        "rbq_profile_begin": (None, [_VP]),
        "rbq_profile_end": (None, [_VP]),
        "rbq_profile_stage_ms": (_F64, [_VP, _STR, _PU64]),
        "rbq_profile_stage_samples": (_U64, [_VP, _STR, _VP, _U64]),
        "rbq_profile_scan_bytes": (_U64, [_VP]),
        "rbq_profile_counters": (_INT, [_VP, _VP, _U32]),
        "rbq_profile_select_stages": (None, [_VP, _U32]),
        "rbq_profile_set_sampling": (None, [_VP, _U32]),
        "rbq_debug_rank_fallbacks": (_U64, [_VP]),
        "rbq_debug_tie_log_stats": (None, [_VP, _VP]),
        "rbq_debug_stage_resources": (_INT, [_VP, _U64, _U32, _U32, _VP]),
        "rbq_debug_bounce_copies": (_U64, []),
        "rbq_debug_head_exact_evaluations": (_U64, [_VP]),
        "rbq_debug_head_exact_guard_trips": (_U64, [_VP]),
        "rbq_debug_heap_restarts": (_U64, [_VP]),
        "rbq_debug_copy_index": (_INT, [_VP, _STR, _VP, _U64]),
        "rbq_debug_best_rescale": (_INT, [_VP, _U64, _U32, _U32, _INT, _VP]),
        "rbq_debug_copy_workspace": (_INT, [_VP, _VP, _STR, _VP, _U64]),
        "rbq_debug_set_option": (_INT, [_VP, _STR, _INT]),
        "rbq_process_defaults": (_INT, []),
        "rbq_strerror": (_STR, [_INT]),
        "rbq_last_error_detail": (_INT, [_STR, _SZ]),
        "rbq_abi_version": (_U32, []),
    },
    # include/rbq_bf.h
    "rbq_bf.h": {
        "rbq_bf_create": (_INT, [_VP, _VP, _INT, _OUT]),
        "rbq_bf_train_device": (_INT, [_VP, _VP, _U64, _INT, _F32, _U64, _INT, _OUT]),
        "rbq_bf_load_rbf1": (_INT, [_VP, _SZ, _INT, _OUT]),
        "rbq_bf_save_rbf1": (_INT, [_VP, _BYTES, _PU64]),
        "rbq_bf_free_bytes": (None, [C.POINTER(_U8)]),
        "rbq_bf_destroy": (None, [_VP]),
        "rbq_bf_len": (_U64, [_VP]),
        "rbq_bf_dim": (_U32, [_VP]),
        "rbq_bf_padded_dim": (_U32, [_VP]),
        "rbq_bf_search_batch": (_INT, [_VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _VP, _VP]),
        "rbq_bf_debug_heap_stats": (None, [_VP, _VP]),
        "rbq_bf_debug_set_chunk_vectors": (_U64, [_U64]),
        "rbq_bf_debug_select_launches": (_U64, []),
    },
    # include/rbq_bf_mutate.h
    "rbq_bf_mutate.h": {
        "rbq_bf_append": (_INT, [_VP, _VP, _U64, _INT, _F32, _U64, _OUT]),
        "rbq_bf_remove_ids": (_INT, [_VP, _VP, _U64, _PU64, _OUT]),
        "rbq_bf_fetch_embeddings": (_INT, [_VP, _VP, _U64, _VP, _VP]),
        "rbq_bf_fetch_embeddings_device": (_INT, [_VP, _VP, _U64, _VP, _VP, _VP]),
        "rbq_bf_debug_append_carry_ns": (_U64, []),
        "rbq_bf_debug_remove_gather_ns": (_U64, []),
    },
    # include/rbq_kmeans.h
    "rbq_kmeans.h": {
        "rbq_kmeans_device": (_INT, [_VP, _U64, _U32, _U64, _U64, _U64, _U64, _INT, _U64, _U64, _INT, _VP, _VP, C.POINTER(_F64), _VP]),
        "rbq_debug_set_kmeans_chunk_rows": (_U64, [_U64]),
        "rbq_debug_kmeans_assign_passes": (_U64, []),
        "rbq_debug_gemm_shortlist_front": (_INT, [_VP, _U64, _U32, _VP, _U64, _INT, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    },
    # include/rbq_persist.h
    "rbq_persist.h": {
        "rbq_index_create_with_recon": (_INT, [_VP, _VP, _VP, _VP, _INT, _VP, _OUT]),
        "rbq_index_save_rbq1_stream": (_INT, [_VP, WRITE_FN, _VP]),
        "rbq_index_save_rbq1": (_INT, [_VP, _BYTES, _PU64]),
        "rbq_persist_free_bytes": (None, [C.POINTER(_U8)]),
        "rbq_debug_crc32_device": (_INT, [_VP, _U64, _INT, C.POINTER(_U32)]),
        "rbq_index_load_rbq1_stream": (_INT, [READ_FN, _VP, _U64, _INT, _VP, _OUT]),
        "rbq_debug_set_load_span": (_U64, [_U64]),
    },
    # include/rbq_append.h
    "rbq_append.h": {
        "rbq_index_append": (_INT, [_VP, _VP, _VP, _U64, _U64, _INT, _F32, _U64, _INT, _VP, _VP, _OUT]),
        "rbq_index_id_bound": (_INT, [_VP, _PU64]),
        "rbq_debug_append_passes": (_U64, []),
        "rbq_debug_append_carry_ns": (_U64, []),
    },
    # include/rbq_remove.h
    "rbq_remove.h": {
        "rbq_index_remove_ids": (_INT, [_VP, _VP, _U64, _INT, _VP, _PU64, _OUT]),
        "rbq_debug_remove_gather_ns": (_U64, []),
    },
    # include/rbq_mstg.h
    "rbq_mstg.h": {
        "rbq_mstg_closure_assign": (_INT, [_VP, _U64, _U32, _VP, _U64, _F32, _U32, _U64, _INT, _VP, _VP]),
        "rbq_mstg_build_device": (_INT, [_VP, _VP, _VP, _U64, _F32, _U32, _INT, _F32, _U64, _INT, _OUT]),
        "rbq_mstg_cluster_device": (_INT, [_VP, _U64, _U32, _U64, _U64, _F32, _U64, _U64, _INT, _OUT]),
        **HCLUSTERED,
        "rbq_mstg_debug_closure_fallbacks": (_U64, []),
        "rbq_mstg_debug_closure_shortlist": (_INT, [_VP, _U64, _U32, _VP, _U64, _U32, _U64, _INT, _VP, _VP]),
        "rbq_mstg_search_batch": (_INT, [_VP, _VP, _U64, _U32, _U32, _U32, _F32, _VP, _VP, _VP, _VP, _VP]),
        "rbq_mstg_search_batch_device": (_INT, [_VP, _VP, _U64, _U32, _U32, _U32, _F32, _VP, _VP, _VP, _VP, _VP, _VP]),
        "rbq_mstg_search_refined_batch": (_INT, [_VP, _VP, _U64, _U32, _U32, _U32, _F32, _U32, _VP, _VP, _VP, _VP, _VP]),
        "rbq_mstg_search_refined_batch_device": (_INT, [_VP, _VP, _U64, _U32, _U32, _U32, _F32, _U32, _VP, _VP, _VP, _VP, _VP, _VP]),
        "rbq_mstg_debug_search_fallbacks": (_U64, []),
    },
    # include/rbq_mstg_persist.h
    "rbq_mstg_persist.h": {
        "rbq_mstg_save_stream": (_INT, [_VP, _VP, WRITE_FN, _VP]),
        "rbq_mstg_save": (_INT, [_VP, _VP, _BYTES, _PU64]),
        "rbq_mstg_load": (_INT, [_VP, _U64, _INT, _VP, _OUT]),
        "rbq_mstg_load_stream": (_INT, [READ_FN, _VP, _U64, _INT, _VP, _OUT]),
        "rbq_mstg_memory_usage": (_U64, [_VP]),
    },
    # include/rbq_mstg_mutate.h
    "rbq_mstg_mutate.h": {
        "rbq_mstg_append": (_INT, [_VP, _VP, _U64, _U64, _F32, _U32, _U64, _VP, _VP, _OUT]),
        "rbq_mstg_remove_ids": (_INT, [_VP, _VP, _U64, _PU64, _OUT]),
        "rbq_debug_mstg_append_passes": (_U64, []),
    },
}
LIBRBQ = {name: proto for group in LIBRBQ_BY_HEADER.values() for name, proto in group.items()}

# csrc/host/rbq_build.h
LIBRBQ_BUILD = {
    "rbq_build_train_with_clusters": (_INT, [_VP, _U64, _U32, _VP, _U64, _VP, _U32, _U8, _U8, _U64, _INT, _OUT]),
    "rbq_built_header": (C.POINTER(Header), [_VP]),
    "rbq_built_lists": (C.POINTER(ListView), [_VP]),
    "rbq_built_t_const": (_F32, [_VP]),
    "rbq_built_list_recon": (_INT, [_VP, _U64, C.POINTER(C.POINTER(_F32)), C.POINTER(C.POINTER(_F32))]),
    "rbq_built_list_residual_norm": (_INT, [_VP, _U64, C.POINTER(C.POINTER(_F32))]),
    "rbq_built_free": (None, [_VP]),
    "rbq_built_save_rbq1": (_INT, [_VP, _BYTES, _PU64]),
    "rbq_build_free_bytes": (None, [C.POINTER(_U8)]),
    "rbq_build_mstg_file_check": (_INT, [_VP, _U64, _STR, _U64, C.POINTER(MstgConfig), _VP]),
    "rbq_build_best_rescale_factor": (_F64, [_VP, _U64, _U32]),
    "rbq_build_pack_binary_code": (None, [_VP, _VP, _U64]),
    "rbq_build_pack_ex_code_1bit": (None, [_VP, _VP, _U64]),
    "rbq_build_pack_ex_code_2bit": (None, [_VP, _VP, _U64]),
    "rbq_build_pack_ex_code_6bit": (None, [_VP, _VP, _U64]),
    "rbq_build_pack_codes": (None, [_VP, _U64, _U64, _VP]),
    "rbq_build_crc32": (_U32, [_VP, _U64]),
    "rbq_build_rotate": (None, [C.POINTER(Header), _VP, _VP]),
    "rbq_build_kmeans": (_INT, [_VP, _U64, _U32, _U64, _INT, _U64, _VP, _VP]),
    "rbq_build_kmeans_faiss": (_INT, [_VP, _U64, _U32, _U64, _U64, _U64, _U64, _INT, _U64, _U64, _VP, _VP, C.POINTER(_F64), _VP]),
    "rbq_build_train_bruteforce": (_INT, [_VP, _U64, _U32, _U32, _U8, _U8, _U64, _INT, _OUT]),
    "rbq_bf_built_header": (C.POINTER(Header), [_VP]),
    "rbq_bf_built_view": (C.POINTER(BfView), [_VP]),
    "rbq_bf_built_t_const": (_F32, [_VP]),
    "rbq_bf_built_free": (None, [_VP]),
    "rbq_build_closure_assign": (_INT, [_VP, _U64, _U32, _VP, _U64, _F32, _U32, _VP, _VP]),
    "rbq_build_mstg_select_lists": (_INT, [_VP, _U64, _U32, _VP, _U64, _U32, _F32, _VP, _VP]),
    "rbq_build_hcluster": (_INT, [_VP, _U64, _U32, _U64, _U64, _F32, _U64, _OUT, C.POINTER(_STR)]),
    **HCLUSTERED,
}


def bind(L, table):
    """Declare restype and argtypes of every function of `table` on the loaded library `L` (a missing symbol is an AttributeError)."""
    for name, (restype, argtypes) in table.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L
