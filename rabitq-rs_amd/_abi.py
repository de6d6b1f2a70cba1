"""ctypes mirror of include/rbq.h (plain data-contract structs + error codes)."""
import ctypes as C

RBQ_OK, RBQ_DIMENSION_MISMATCH, RBQ_INVALID_CONFIG, RBQ_EMPTY_INDEX, RBQ_IO, \
    RBQ_INVALID_PERSISTENCE, RBQ_DEVICE = range(7)
METRIC_L2, METRIC_IP = 0, 1
ROTATOR_MATRIX, ROTATOR_FHT_KAC = 0, 1
# numeric variants (RBQ_NUMERIC_*): which build of the reference the scores reproduce bit for bit
NUMERIC_NATIVE_AVX512, NUMERIC_NATIVE_AVX2, NUMERIC_PORTABLE = 0, 1, 2
NUMERIC_VARIANTS = {"native_avx512": NUMERIC_NATIVE_AVX512, "native_avx2": NUMERIC_NATIVE_AVX2, "portable": NUMERIC_PORTABLE}
# rescale modes of the device encoder (RBQ_RESCALE_*): RabitqConfig::faster / RabitqConfig::new
RESCALE_CONST, RESCALE_OPTIMAL = 0, 1
RESCALE_MODES = {"const": RESCALE_CONST, "optimal": RESCALE_OPTIMAL}
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


# include/rbq_mstg_mutate.h: (restype, argtypes) of every entry point, argument for argument (index.lib() applies them)
_VP, _U64, _U32 = C.c_void_p, C.c_uint64, C.c_uint32
MSTG_MUTATE_PROTOTYPES = {
    # idx, vectors, count, first_id, closure_epsilon, max_replicas, max_chunk_rows, out_lists, out_counts, out
    "rbq_mstg_append": (C.c_int, [_VP, _VP, _U64, _U64, C.c_float, _U32, _U64, _VP, _VP, C.POINTER(_VP)]),
    # idx, ids, n_ids, out_removed, out
    "rbq_mstg_remove_ids": (C.c_int, [_VP, _VP, _U64, C.POINTER(_U64), C.POINTER(_VP)]),
    "rbq_debug_mstg_append_passes": (_U64, []),
}
