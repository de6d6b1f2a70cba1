"""Cases of the call-sequence tests: four small indexes, a literal catalogue of call kinds, the CPU
reference of every kind (the project's existing references, nothing new) and the comparison each feature's own test applies.
tests/test_call_sequence_cases_host.py shows on the CPU that the catalogue is not hollow; tests/test_gpu_call_sequences.py runs
every kind alone, after every other kind, in unsynchronised chains, on two streams and through the host entry, and asks that a
call's result never depends on the calls the handle served before."""
import functools
from typing import NamedTuple

import numpy as np

import oracle
import range_exact_ref
import range_ref
import rerank_f16_ref
import rerank_pool_ref
from conftest import build_index, make_dataset

F32 = np.float32
PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_BITS = np.uint32(0x7FC00000)
FILL = 0x5A  # every output buffer is filled with this byte before a call: padding the kernels did not write is seen
VARIANT_MASK = {"native_avx2": 1, "portable": 6}  # the oracle's mask of a numeric variant (tests/test_gpu_numeric_variant.py)
QUERY_DTYPE = {0: "f32", 1: "f16", 2: "bf16"}     # RBQ_RAW_* of the option "query_dtype"


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1. the indexes -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    data: np.ndarray      # the raw vectors (attached for the rerank on A and B)
    built: object
    q: np.ndarray         # the query set, f32
    extra: dict           # A: "deg" = the degenerate rows; P: "lists", "counts"


def _index_a():
    """FHT-Kac, dim 384 (12 K slabs, a compile-time DT, D % 64 == 0: the split routes, the latency kernel), 7 bits, L2, 24 lists.
    Rows 5998 / 5999 duplicate rows 101 / 100 and queries 0 / 1 sit beside them: two equal distances at the head of their top-k.
    Query 699 is far from everything (no match at any radius taken from another query)."""
    n, dim, nlist = 6000, 384, 24
    data = make_dataset(n, dim, 6, 3401)
    data[5998], data[5999] = data[101], data[100]
    _, built = build_index(nlist=nlist, total_bits=7, metric=0, rotator=1, seed=3402, data=data)
    rng = np.random.default_rng(3403)
    q = make_dataset(700, dim, 6, 3404)
    q[0] = data[100] + F32(0.01) * rng.standard_normal(dim).astype(F32)
    q[1] = data[101] + F32(0.01) * rng.standard_normal(dim).astype(F32)
    q[699] = data.mean(0) + F32(25.0)
    deg = make_dataset(8, dim, 6, 3405)  # the forms of tests/test_gpu_round4.py::test_degenerate_queries
    deg[0] = 0.0
    deg[1, 5] = np.nan
    deg[2] = np.nan
    deg[3, 7] = np.inf
    deg[4] = np.inf
    deg[5] = data[100]
    deg[6] = -0.0
    return Case("A", data, built, np.ascontiguousarray(q, F32), {"deg": np.ascontiguousarray(deg, F32)})


def _index_b():
    """matrix rotator, dim 96 (D % 64 != 0: the f32 GEMM, k_prep, the runtime-dimension scan), 3 bits, inner product on
    normalised data, 12 lists.  Query 699 is a hundredth of query 1: every score of it is a hundredth of a usual one."""
    data, built = build_index(n=3000, dim=96, nlist=12, total_bits=3, metric=1, rotator=0, seed=3411, normalize=True)
    q = make_dataset(700, 96, 3, 3412, normalize=True)
    q[699] = F32(0.01) * q[1]
    return Case("B", data, built, np.ascontiguousarray(q, F32), {})


def _index_c():
    """FHT-Kac, dim 16 (padded to 64), 1 bit, L2, 8200 lists of two vectors: above 8192 lists nprobe can exceed kNprobeMax (big_nprobe, the key
    window in global memory).  Vector v in list v % n_lists around seeded centroids, as tools/route_dump.py builds its indexes."""
    import rabitq_rs_amd as rq
    n, dim, nlist = 16400, 16, 8200
    rng = np.random.default_rng(3421)
    cent = rng.standard_normal((nlist, dim)).astype(F32)
    assign = (np.arange(n) % nlist).astype(np.uint32)
    data = cent[assign] + F32(0.25) * rng.standard_normal((n, dim)).astype(F32)
    built = rq.builder.train_with_clusters(data, cent, assign, 1, 0, 1, 3422, True)
    q = data[rng.choice(n, 9, replace=False)] + F32(0.05) * rng.standard_normal((9, dim)).astype(F32)
    return Case("C", data, built, np.ascontiguousarray(q, F32), {})


def _index_p():
    """a posting-list handle (RBQ_ROTATOR_NONE): _mstg_case of tests/test_gpu_parity.py, 7 bits, L2"""
    from test_gpu_parity import _mstg_case
    built, q, lists, counts = _mstg_case(0, 7)
    return Case("P", None, built, np.ascontiguousarray(q, F32), {"lists": lists, "counts": counts})


@functools.lru_cache(maxsize=None)
def case(name):
    return {"A": _index_a, "B": _index_b, "C": _index_c, "P": _index_p}[name]()


@functools.lru_cache(maxsize=None)
def allowed_ids(index):
    """about 30 % of the ids"""
    n = len(case(index).data)
    return frozenset(int(i) for i in np.nonzero(np.random.default_rng(3430).random(n) < 0.3)[0])


def filter_of(kind):
    """(allowed set | None, filter words | None, filter bits) of a kind: "30" = 30 % of the ids in as many bits as there are ids,
    "short" = the same ids in a filter of half the id space"""
    if kind.filt is None:
        return None, None, 0
    n = len(case(kind.index).data)
    nbits = n if kind.filt == "30" else n // 2
    keep = frozenset(i for i in allowed_ids(kind.index) if i < nbits)
    w = np.zeros((nbits + 31) // 32, np.uint32)
    a = np.array(sorted(keep), np.uint64)
    np.bitwise_or.at(w, (a >> np.uint64(5)).astype(np.int64), (np.uint32(1) << (a & np.uint64(31)).astype(np.uint32)))
    return keep, w, nbits


# ---- 2. the catalogue -------------------------------------------------------------------------------------------------------------
class Kind(NamedTuple):
    name: str
    index: str     # "A", "B", "C" or "P"
    rows: tuple    # (first row, rows) of the index's query set; ("deg", rows) = A's degenerate rows
    top_k: int     # (range modes: the capacity of a row; 0 = the largest total of the reference + 3)
    nprobe: int    # (posting: max_lists)
    filt: object   # None, "30" or "short"
    diag: bool
    entry: str     # "device" (rbq_search_batch_device on a caller stream) or "host" (rbq_search_batch, pageable buffers)
    opts: tuple    # ((option, value for the call, value put back after it), ...); "numeric_variant" goes through its own setter
    mode: str      # "topk", "range", "range_exact", "rerank", "rerank_pool" or "posting"
    arg: object    # range: (k, row): the radius is query `row`'s k-th distance; range_exact: (k of the exact x, k of the estimate's r, row)
    why: str       # the route of the DESIGN section 31 table, or the workspace buffer, the kind is there for


def K(name, index, first, nq, top_k, nprobe, why, filt=None, diag=False, entry="device", opts=(), mode="topk", arg=None):
    return Kind(name, index, (first, nq), top_k, nprobe, filt, diag, entry, tuple(opts), mode, arg, why)


F16, BF16 = ("query_dtype", 1, 0), ("query_dtype", 2, 0)
RERANK = ("rerank", 1, 0)

# Every kind reads rows of its own (or differs in top_k / nprobe / filter from the kinds it shares rows with), so that no two
# references of an index are equal: a stale read of the other call's data cannot pass as correct.
KINDS = [
    # -- index A: the fronts and the preparations ---------------------------------------------------------------------------------
    K("a_nq1", "A", 0, 1, 10, 6, "latency front (k_lat_front with its scorers, no ranking stage) at one query"),
    K("a_nq4", "A", 0, 4, 10, 6, "latency front at its last batch size; scores rows of 4 queries"),
    K("a_nq5", "A", 4, 5, 10, 6, "one past the latency front: the latency kernel as preparation only, clearing (wg_zero), split-K"),
    K("a_nq200", "A", 10, 200, 10, 6, "split-K (2 parts of 6 K slabs) ADDS into the score rows the wg_zero preparation clears; k_scanw"),
    K("a_nq200_ksplit0", "A", 20, 200, 10, 6, "the unsplit GEMM overwrites `scores` behind the plain wg preparation", opts=[("rank_ksplit", 0, 1)]),
    K("a_nq200_ksplit4", "A", 30, 200, 10, 6, "forced 4 parts of 3 K slabs into cleared `scores`", opts=[("rank_ksplit", 4, 1)]),
    K("a_nq513", "A", 40, 513, 10, 6, "one past kPrepWgMaxQueries: k_prep_wave, no split-K, k_scanw on the device entry"),
    K("a_nq700", "A", 0, 700, 10, 6, "k_prep_wave and k_scanw at the full query set: rows of every per-query buffer up to 700"),
    K("a_nq200_wgprep", "A", 50, 200, 10, 6, "k_prep (option wg_prep): never clears `scores`, so no split-K", opts=[("wg_prep", 1, 0)]),
    K("a_nq200_lat0", "A", 60, 200, 10, 6, "latency_path 0: k_prep_wave below 512 queries, `scores` not cleared, no split-K", opts=[("latency_path", 0, 1)]),
    K("a_tile128", "A", 70, 200, 10, 6, "rank_tile 128 forced (by rule it needs 192 tiles): split-K on the 128 tile", opts=[("rank_tile", 128, 0)]),
    K("a_tile256", "A", 80, 200, 10, 6, "rank_tile 256 forced (by rule 2048 tiles): parts were decided, the 256 grid has no z, the rows are cleared anyway",
      opts=[("rank_tile", 256, 0)]),
    # -- the ranking routes, each at nq 64 ------------------------------------------------------------------------------------------
    K("a_exact_rank", "A", 100, 64, 10, 6, "exact route: k_rank_scores + k_select; the scan gets no `dead_skipped`", opts=[("exact_rank", 1, 0)]),
    K("a_rank_fallback", "A", 101, 64, 10, 6, "k_select_mfma's canonical fallback for every row of `scores`", opts=[("force_rank_fallback", 1, 0)]),
    K("a_f32_rank", "A", 102, 64, 10, 6, "k_rank_mfma (f32 GEMM) on an index that would split: `rot_hl` unused", opts=[("f32_rank", 1, 0)]),
    K("a_rank_planar", "A", 103, 64, 10, 6, "planar operand copies in `rank_planes` ((nq + n_lists) x D, offsets move with nq)", opts=[("rank_planar", 1, 0)]),
    K("a_rank_f16", "A", 104, 64, 10, 6, "one f16 product: `rot_f16`, `rank_resid` (rank_ksplit 0 with it: at 64 queries the parts decided by rule exclude the f16 route)",
      opts=[("rank_f16", 1, -1), ("rank_ksplit", 0, 1)]),
    # -- the scan kernels -------------------------------------------------------------------------------------------------------------
    K("a_scan0_k10", "A", 110, 64, 10, 6, "k_scan by option; `tie_log` at 2048 entries per query", opts=[("scan_wave", 0, -1)]),
    K("a_scan0_k100", "A", 111, 64, 100, 6, "k_scan, TR 2; `tie_log` at 8192 entries per query", opts=[("scan_wave", 0, -1)]),
    K("a_scan1_k10", "A", 112, 64, 10, 6, "k_scanw by option below 128 queries, TR 1; no tie log", opts=[("scan_wave", 1, -1)]),
    K("a_scan1_k100", "A", 113, 64, 100, 6, "k_scanw, TR 2", opts=[("scan_wave", 1, -1)]),
    K("a_scan2_k10", "A", 114, 64, 10, 6, "scan_wave 2 set explicitly: k_scan below 128 queries", opts=[("scan_wave", 2, -1)]),
    K("a_scan2_k100", "A", 115, 64, 100, 6, "scan_wave 2 set explicitly, top_k 100", opts=[("scan_wave", 2, -1)]),
    K("a_nq128_k129", "A", 116, 128, 129, 6, "k_scanw from 128 queries by rule, TR 4"),
    K("a_lazy_diag", "A", 119, 64, 10, 24, "lazy k_select_mfma with diagnostics over every list: whole lists dropped, `dead_skipped` non-zero", diag=True),
    K("a_lazy0", "A", 120, 64, 10, 6, "eager k_select_mfma: `dead_skipped` is still passed to the scan and added to the diagnostics: it must read zero",
      opts=[("lazy_select", 0, 1)], diag=True),
    K("a_block_bound0", "A", 121, 64, 10, 6, "block bound off: eager selection, every probed block streamed (`wl` rows full), `dead_skipped` zero",
      opts=[("block_bound", 0, 1)], diag=True),
    K("a_exact_heap", "A", 0, 64, 10, 6, "exact_heap 1: ties replay the lists, no `tie_log`; queries 0 / 1 have equal distances", opts=[("exact_heap", 1, 0)]),
    K("a_tie_log0", "A", 0, 64, 11, 6, "tie_log 0: a tied query is scanned again; queries 0 / 1 have equal distances", opts=[("tie_log", 0, 1)]),
    # -- top_k: the register forms, the LDS heap, the heap in global memory -------------------------------------------------------
    K("a_k1", "A", 130, 64, 1, 6, "top_k 1 in registers (TR 1); the output stride is 1"),
    K("a_k63", "A", 131, 64, 63, 6, "last top_k of TR 1"),
    K("a_k64", "A", 132, 64, 64, 6, "first top_k of TR 2; `tie_log` 8192 entries per query"),
    K("a_k129", "A", 133, 64, 129, 6, "first top_k of TR 4"),
    K("a_k256", "A", 134, 64, 256, 6, "last top_k in registers"),
    K("a_k300", "A", 135, 16, 300, 6, "the exact heap in LDS, no tie log"),
    K("a_k1000", "A", 136, 16, 1000, 6, "the exact heap in LDS; rows of 1500 probed vectors fill it"),
    K("a_k16400", "A", 137, 3, 16400, 24, "above kTopKMax: `heap_ws` at a stride of 16 401; 6000 vectors, so no row is full"),
    K("a_k17000", "A", 138, 3, 17000, 24, "`heap_ws` at a stride of 17 001 on the rows 16 401 left"),
    # -- nprobe ---------------------------------------------------------------------------------------------------------------------------
    K("a_p1", "A", 140, 32, 10, 1, "nprobe 1: the shortest `probe` / `wl` rows"),
    K("a_p6", "A", 141, 32, 10, 6, "nprobe 6 at 32 queries"),
    K("a_p24", "A", 142, 32, 10, 24, "every list: the longest `probe` / `wl` rows"),
    K("a_p27", "A", 143, 32, 10, 27, "nprobe above n_lists, clamped to 24"),
    # -- filters ------------------------------------------------------------------------------------------------------------------------
    K("a_filter_diag", "A", 150, 64, 10, 6, "a filter with diagnostics: eager selection, every candidate's bit tested", filt="30", diag=True),
    K("a_filter", "A", 151, 64, 10, 6, "a filter without diagnostics: lazy selection on the exact head evaluation", filt="30"),
    K("a_filter_short", "A", 152, 64, 10, 6, "a filter shorter than the id space", filt="short"),
    # -- range search (k_range; eager selection, no heap, no tie log) ------------------------------------------------------------------
    K("a_range21", "A", 636, 64, 0, 6, "k_range at the radius of query 636's 21st distance, capacity above every total", mode="range", arg=(21, 636), diag=True),
    K("a_range50", "A", 636, 64, 0, 6, "k_range at the 50th distance, capacity above every total", mode="range", arg=(50, 636)),
    K("a_range50_cap8", "A", 636, 64, 8, 6, "k_range at a capacity below the totals: rows are cut, totals are not", mode="range", arg=(50, 636)),
    K("a_range50_nq16", "A", 684, 16, 0, 6, "k_range at the same radius, 16 rows", mode="range", arg=(50, 636), diag=True),
    K("a_range50_nq236", "A", 464, 236, 40, 6, "k_range at the same radius, 236 rows of capacity 40: some cut, some not", mode="range", arg=(50, 636)),
    K("a_range_filter", "A", 636, 64, 0, 6, "k_range under a filter", mode="range", arg=(50, 636), filt="30", diag=True),
    K("a_range_exact", "A", 668, 32, 0, 6, "k_range's exact variant: raw rows decide, the caller's queries are read again",
      mode="range_exact", arg=(21, 50, 668), opts=[RERANK], diag=True),
    # -- rerank ---------------------------------------------------------------------------------------------------------------------------
    K("a_rerank", "A", 160, 64, 10, 6, "the unpooled rerank re-scores the returned ids in place", mode="rerank", opts=[RERANK]),
    K("a_rerank_pool64", "A", 161, 64, 10, 6, "pooled rerank: the inner call writes `rr_ids` / `rr_est` / `rr_counts` at a stride of 64", mode="rerank_pool",
      opts=[RERANK, ("rerank_pool", 64, 0)]),
    K("a_rerank_pool300", "A", 162, 48, 10, 1, "pooled rerank at a stride of 300 over ONE list (the inner call on the LDS heap): `rr_counts` differs from row to row", mode="rerank_pool",
      opts=[RERANK, ("rerank_pool", 300, 0)]),
    K("a_rerank_pool300_k290", "A", 163, 48, 290, 1, "the same pool at top_k 290: rows whose list holds fewer than 290 vectors end at their own `rr_counts` entry",
      mode="rerank_pool", opts=[RERANK, ("rerank_pool", 300, 0)]),
    # -- 16-bit queries -------------------------------------------------------------------------------------------------------------------
    K("a_f16_nq5", "A", 170, 5, 10, 6, "f16 queries through the latency kernel as preparation", opts=[F16]),
    K("a_f16_nq64", "A", 171, 64, 10, 6, "f16 queries, 64 rows of half the bytes", opts=[F16]),
    K("a_bf16_nq5", "A", 172, 5, 10, 6, "bf16 queries through the latency kernel as preparation", opts=[BF16]),
    K("a_bf16_nq64", "A", 173, 64, 10, 6, "bf16 queries", opts=[BF16]),
    # -- numeric variants: the runtime-dimension scan only --------------------------------------------------------------------------
    K("a_avx2", "A", 180, 64, 10, 6, "native_avx2: the runtime-dimension k_scan", opts=[("numeric_variant", "native_avx2", "native_avx512")]),
    K("a_portable", "A", 181, 64, 10, 6, "portable: the runtime-dimension k_scan, scalar epilogue", opts=[("numeric_variant", "portable", "native_avx512")]),
    # -- degenerate rows and the widest call ------------------------------------------------------------------------------------------
    K("a_degenerate", "A", "deg", 8, 10, 6, "zero, NaN and +inf queries: non-finite rows of `rot`, `lut`, `consts`, `scores` left behind", diag=True),
    K("a_widest", "A", 0, 700, 256, 24, "the widest call: fills every per-query buffer at its longest stride", diag=True),
    # -- the host entry (pool lanes, staging buffers) -------------------------------------------------------------------------------------
    K("a_host_nq8_sub3", "A", 190, 8, 10, 6, "host entry, sub-batches of 3 / 3 / 2 on lanes: `h_in`, `h_out`, call_nq 8", entry="host", opts=[("host_subbatch", 3, 0)]),
    K("a_host_nq700_sub64", "A", 0, 700, 12, 6, "host entry, sub-batches of 64 shrinking towards the end: a lane serves a small one after a full one",
      entry="host", opts=[("host_subbatch", 64, 0)]),
    K("a_host_nq1", "A", 191, 1, 10, 6, "host entry at one query: latency_first, call_nq 1", entry="host"),
    # -- index B ----------------------------------------------------------------------------------------------------------------------------
    K("b_nq1", "B", 0, 1, 10, 2, "matrix rotator: k_prep and the f32 GEMM even at one query"),
    K("b_nq5", "B", 1, 5, 10, 4, "k_prep at 5 queries"),
    K("b_nq64", "B", 10, 64, 10, 4, "k_prep, k_rank_mfma, the runtime-dimension k_scan"),
    K("b_nq600", "B", 20, 600, 10, 4, "the runtime-dimension k_scanw; the longest rows of B"),
    K("b_k300", "B", 30, 16, 300, 4, "the LDS heap at the runtime dimension"),
    K("b_p1", "B", 70, 32, 5, 1, "nprobe 1 at top_k 5: the shortest `probe` / `wl` rows of B"),
    K("b_k100_p8", "B", 90, 32, 100, 8, "top_k 100 (TR 2 at the runtime dimension) over 8 lists"),
    K("b_p12", "B", 80, 8, 20, 12, "every list of B at 8 queries"),
    K("b_filter", "B", 40, 64, 10, 4, "a filter under inner product", filt="30", diag=True),
    K("b_range", "B", 636, 64, 0, 4, "the runtime-dimension k_range under inner product", mode="range", arg=(50, 636), diag=True),
    K("b_range_cap60", "B", 600, 36, 60, 4, "the same radius at 36 rows of capacity 60: some cut, some not", mode="range", arg=(50, 636)),
    K("b_rerank_pool", "B", 50, 64, 10, 4, "pooled rerank under inner product", mode="rerank_pool", opts=[RERANK, ("rerank_pool", 64, 0)]),
    K("b_f16", "B", 60, 64, 10, 4, "f16 queries through k_prep", opts=[F16]),
    # -- index C ----------------------------------------------------------------------------------------------------------------------------
    K("c_big_nq3", "C", 0, 3, 10, 8200, "big_nprobe: exact route, `key_window` of 3 rows in global memory"),
    K("c_big_nq9", "C", 0, 9, 10, 8200, "big_nprobe: `key_window` of 9 rows"),
    K("c_p100", "C", 0, 9, 12, 100, "8200 lists below kNprobeMax (dim 16 is padded to 64: the split GEMM, 129 tiles of 64 lists): k_select_mfma over long `scores` rows"),
    K("c_exact_rank", "C", 0, 9, 11, 100, "exact route by option: k_select with the key window in LDS", opts=[("exact_rank", 1, 0)]),
    # -- index P: posting_scan (`nprobe` = max_lists; the list counts of row 0 are 0) -----------------------------------------------
    K("p_k1", "P", 0, 40, 1, 12, "posting scan, top_k 1", mode="posting"),
    K("p_k10", "P", 0, 40, 10, 12, "posting scan, top_k 10", mode="posting"),
    K("p_k100", "P", 0, 40, 100, 12, "posting scan, top_k 100", mode="posting"),
    K("p_k300", "P", 0, 40, 300, 12, "posting scan on the LDS heap", mode="posting"),
    K("p_k10_m5", "P", 0, 40, 10, 5, "posting scan at a list stride of 5", mode="posting"),
    K("p_k100_m5", "P", 0, 17, 100, 5, "posting scan at a list stride of 5, 17 rows", mode="posting"),
    K("p_k10_nq7", "P", 0, 7, 10, 12, "posting scan of 7 rows, the first without a list", mode="posting"),
    K("p_k10_tail", "P", 21, 19, 10, 12, "posting scan of the last 19 rows: every row has a list", mode="posting"),
]
BY_NAME = {k.name: k for k in KINDS}
assert len(BY_NAME) == len(KINDS)


def kinds_of(index):
    return [k for k in KINDS if k.index == index]


def plain(kind):
    """a kind that needs no option change: only nq, top_k, nprobe, the filter and the diagnostics vary (the unsynchronised chains)"""
    return kind.entry == "device" and not kind.opts and kind.mode == "topk"


def range_chain(index):
    """the range kinds of an index that need no option change once the radius of (50, 636) is set: capacities, nq and the filter vary"""
    return [k for k in kinds_of(index) if k.mode == "range" and k.arg == (50, 636) and not k.opts]


# What rbq_debug_stage_resources must report for a kind on the device entry, where the probe can tell routes apart:
# "prep" = workgroups of the preparation (k_lat_front with scorers: 8 per query at 24 lists; workgroup forms and k_prep: one per query;
# k_prep_wave: one per four queries), "rank" = the ranking stage's operands (None: no ranking stage), "parts" = the ranking GEMM's
# workgroups as a multiple of the same call's under rank_ksplit 0, "scan" = threads of the scan (64 k_scanw, 256 k_scan / k_range).
ROUTES = {
    "a_nq1": {"prep": 8, "rank": None, "scan": 256},
    "a_nq4": {"prep": 32, "rank": None, "scan": 256},
    "a_nq5": {"prep": 5, "rank": "bf16x3", "parts": 2, "scan": 256},
    "a_nq200": {"prep": 200, "rank": "bf16x3", "parts": 2, "scan": 64},
    "a_nq200_ksplit0": {"prep": 200, "rank": "bf16x3", "parts": 1, "scan": 64},
    "a_nq200_ksplit4": {"prep": 200, "rank": "bf16x3", "parts": 4, "scan": 64},
    "a_nq513": {"prep": 129, "rank": "bf16x3", "parts": 1, "scan": 64},
    "a_nq700": {"prep": 175, "rank": "bf16x3", "parts": 1, "scan": 64},
    "a_nq200_wgprep": {"prep": 200, "rank": "bf16x3", "parts": 1, "scan": 64},
    "a_nq200_lat0": {"prep": 50, "rank": "bf16x3", "parts": 1, "scan": 64},
    "a_tile128": {"prep": 200, "rank": "bf16x3", "parts": 2, "scan": 64},
    "a_tile256": {"prep": 200, "rank": "bf16x3", "scan": 64},
    "a_exact_rank": {"prep": 64, "rank": "f32", "scan": 256},
    "a_rank_fallback": {"prep": 64, "rank": "bf16x3", "parts": 2, "scan": 256},
    "a_f32_rank": {"prep": 64, "rank": "f32", "parts": 1, "scan": 256},
    "a_rank_planar": {"prep": 64, "rank": "bf16x3", "parts": 2, "scan": 256},
    "a_rank_f16": {"prep": 64, "rank": "f16", "scan": 256},
    "a_scan0_k10": {"scan": 256}, "a_scan0_k100": {"scan": 256}, "a_scan1_k10": {"scan": 64}, "a_scan1_k100": {"scan": 64},
    "a_scan2_k10": {"scan": 256}, "a_scan2_k100": {"scan": 256}, "a_nq128_k129": {"scan": 64},
    "a_block_bound0": {"scan": 256}, "a_range50_nq236": {"prep": 236, "scan": 256}, "a_k256": {"scan": 256}, "a_k300": {"scan": 256}, "a_k16400": {"scan": 256},
    "a_range21": {"prep": 64, "scan": 256}, "a_range_exact": {"scan": 256},
    "a_avx2": {"scan": 256}, "a_portable": {"scan": 256},
    "a_widest": {"prep": 175, "rank": "bf16x3", "parts": 1, "scan": 256},
    "b_nq1": {"prep": 1, "rank": "f32", "scan": 256},
    "b_nq5": {"prep": 5, "rank": "f32", "scan": 256},
    "b_nq64": {"prep": 64, "rank": "f32", "scan": 256},
    "b_nq600": {"prep": 600, "rank": "f32", "scan": 64},
    "b_range": {"prep": 64, "rank": "f32", "scan": 256},
    "c_big_nq3": {"prep": 3, "rank": "f32", "scan": 256},
    "c_big_nq9": {"prep": 9, "rank": "f32", "scan": 256},
    "c_p100": {"prep": 9, "rank": "bf16x3", "parts": 1, "scan": 256},
    "c_exact_rank": {"prep": 9, "rank": "f32", "scan": 256},
}
assert set(ROUTES) <= set(BY_NAME)


# ---- 3. queries, radii, references -----------------------------------------------------------------------------------------------
def query_dtype_of(kind):
    for name, value, _ in kind.opts:
        if name == "query_dtype":
            return QUERY_DTYPE[value]
    return "f32"


@functools.lru_cache(maxsize=None)
def _queries(name):
    kind = BY_NAME[name]
    c = case(kind.index)
    first, nq = kind.rows
    q = c.extra["deg"][:nq] if first == "deg" else c.q[first:first + nq]
    assert len(q) == nq
    dt = query_dtype_of(kind)
    if dt == "f32":
        return np.ascontiguousarray(q, F32), np.ascontiguousarray(q, F32)
    h = rerank_f16_ref.round_to(q, dt)  # rounded here, once; the library reads the patterns and widens them exactly
    return np.ascontiguousarray(h), np.ascontiguousarray(rerank_f16_ref.widen(h, dt), F32)


def queries(kind):
    """(the rows handed to the library: f32, or uint16 patterns of f16 / bf16; the f32 values the library reads)"""
    return _queries(kind.name)


def posting_lists(kind):
    c = case("P")
    first, nq = kind.rows
    m = kind.nprobe
    lists = np.ascontiguousarray(c.extra["lists"][first:first + nq, :m])
    return lists, np.minimum(c.extra["counts"][first:first + nq], m).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def radii(name):
    """range: (r,); range_exact: (r of the estimate, x of the exact score) — from one query's k-th distance, as tests/test_gpu_range.py
    and tests/test_gpu_range_exact.py take theirs; kinds that name the same (k, row) share a radius (the range chains set it once)"""
    kind = BY_NAME[name]
    c = case(kind.index)
    if kind.mode == "range":
        k, row = kind.arg
        return (range_ref.kth_distance_radius(c.built, c.q[row], k, kind.nprobe),)
    kx, kr, row = kind.arg
    return (range_ref.kth_distance_radius(c.built, c.q[row], kr, kind.nprobe),
            range_exact_ref.kth_exact_score(c.built, c.q[row], c.data, kx, kind.nprobe))


class Ref(NamedTuple):
    top_k: int          # columns of the result (range modes: the capacity the call is made with)
    ids: np.ndarray     # [nq, top_k] u64, padded with UINT64_MAX
    scores: np.ndarray  # [nq, top_k] f32, padded with the NaN 0x7fc00000
    counts: np.ndarray  # [nq] u32 (range modes: the totals)
    diag: object        # [nq, 3] u64 or None
    probed: object      # range modes: the per-query reference rows; posting: (ids, scores, counts) of the oracle at top_k + 64


@functools.lru_cache(maxsize=None)
def reference(name):
    """The CPU reference of a kind: oracle.search_batch (under oracle.variant for the numeric variants), range_ref.range_batch,
    range_exact_ref, rerank_pool_ref over the oracle's pool, oracle.posting_scan_batch; 16-bit queries enter widened."""
    kind = BY_NAME[name]
    c = case(kind.index)
    wq = queries(kind)[1]
    metric = int(c.built.header.metric)
    keep, fw, nbits = filter_of(kind)
    if kind.mode == "posting":
        lists, counts = posting_lists(kind)
        rc, ids, sc, cnt = oracle.posting_scan_batch(c.built, wq, kind.top_k, lists, counts)
        rc2, xi, xs, xc = oracle.posting_scan_batch(c.built, wq, kind.top_k + 64, lists, counts)
        assert rc == 0 and rc2 == 0
        return Ref(kind.top_k, ids, sc, cnt, None, (xi, xs, xc))
    if kind.mode in ("range", "range_exact"):
        if kind.mode == "range":
            rows = range_ref.range_batch(c.built, wq, radii(name)[0], kind.nprobe, keep)
        else:
            r, x = radii(name)
            rows = range_exact_ref.range_exact_batch(c.built, wq, c.data, x, r, kind.nprobe, keep)
        cap = kind.top_k or max(max(len(r[0]) for r in rows), 1) + 3
        ids, sbits, tot = range_ref.rows(rows, cap)
        return Ref(cap, ids, sbits.view(F32), tot, range_ref.diag_of(rows) if kind.diag else None, rows)
    mask = 0
    for oname, value, _ in kind.opts:
        if oname == "numeric_variant":
            mask = VARIANT_MASK[value]
    inner_k = kind.top_k
    if kind.mode == "rerank_pool":
        inner_k = dict((o[0], o[1]) for o in kind.opts)["rerank_pool"]
    with oracle.variant(mask):
        rc, ids, sc, cnt, diag = oracle.search_batch(c.built, wq, inner_k, kind.nprobe, fw, nbits, want_diag=kind.diag)
    assert rc == 0
    if kind.mode in ("rerank", "rerank_pool"):
        # the pool is the plain search's result at top_k := pool (unpooled: the returned ids themselves), scored exactly and ordered
        # by (exact score, rank in the pool): tests/rerank_pool_ref.py
        ids, sbits, cnt = rerank_pool_ref.rerank_pool(wq, c.data, ids, cnt, metric, kind.top_k)
        sc = sbits.view(F32)
    return Ref(kind.top_k, ids, sc, cnt, diag, None)


# ---- 4. comparisons ----------------------------------------------------------------------------------------------------------------
class Result(NamedTuple):
    ids: np.ndarray     # [nq, top_k] u64
    scores: np.ndarray  # [nq, top_k] f32
    counts: np.ndarray  # [nq] u32
    diag: object        # [nq, 3] u64 or None


def same_bits(got, want, what=""):
    """bit for bit: ids, scores as uint32, counts, diagnostics and padding"""
    assert got.ids.shape == want.ids.shape, f"{what}: shape {got.ids.shape} expected {want.ids.shape}"
    assert np.array_equal(got.counts, want.counts), f"{what}: counts differ for queries {np.nonzero(got.counts != want.counts)[0][:8]}"
    bad = np.nonzero((got.ids != want.ids).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8]}: {got.ids[bad[0]][:8]} expected {want.ids[bad[0]][:8]}"
    bad = np.nonzero((bits(got.scores) != bits(want.scores)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: score bits differ for queries {bad[:8]}: {got.scores[bad[0]][:8]} expected {want.scores[bad[0]][:8]}"
    assert (got.diag is None) == (want.diag is None), what
    if got.diag is not None:
        assert np.array_equal(got.diag, want.diag), f"{what}: SearchDiagnostics differ for queries {np.nonzero((got.diag != want.diag).any(axis=1))[0][:8]}"


def _padding(kind, got, kept, what):
    pad = np.arange(got.ids.shape[1])[None, :] >= kept[:, None]
    assert (got.ids[pad] == PAD_ID).all(), f"{what}: an unused id slot is not UINT64_MAX"
    assert np.isnan(got.scores[pad]).all(), f"{what}: an unused score slot is not NaN"


def check(kind, got, what=None):
    """A kind's result against its reference by the rule of the feature's own test: ids, counts (totals) and diagnostics exactly;
    scores within RTOL of tests/test_gpu_parity.py for the top-k search, by their bits for the numeric variants, range, exact range
    and rerank; the posting scan by its rule about ties at the cut; unused slots UINT64_MAX / NaN."""
    from test_gpu_parity import RTOL
    what = what or kind.name
    ref = reference(kind.name)
    assert got.ids.shape == ref.ids.shape == got.scores.shape, f"{what}: shape {got.ids.shape} expected {ref.ids.shape}"
    if kind.mode == "posting":
        return _check_posting(kind, got, ref, what)
    assert np.array_equal(got.counts, ref.counts), f"{what}: counts {got.counts[:12]} expected {ref.counts[:12]}"
    kept = np.minimum(ref.counts.astype(np.int64), ref.top_k)
    _padding(kind, got, kept, what)
    if kind.diag:
        assert got.diag is not None and np.array_equal(got.diag, ref.diag), f"{what}: SearchDiagnostics differ"
    valid = np.arange(ref.top_k)[None, :] < kept[:, None]
    if kind.mode == "rerank":
        # tests/test_gpu_round2.py::test_optional_rerank_default_off: the same ids, re-scored exactly, in order; an id is
        # determined where its exact score differs from its neighbours' (rows 5998 / 5999 of A duplicate two others)
        assert np.array_equal(bits(got.scores), bits(ref.scores)), f"{what}: exact score bits differ"
        for i in range(len(kept)):
            c = int(kept[i])
            s = bits(ref.scores[i, :c])
            lone = np.ones(c, bool)
            lone[1:] &= s[1:] != s[:-1]
            lone[:-1] &= s[:-1] != s[1:]
            assert np.array_equal(got.ids[i, :c][lone], ref.ids[i, :c][lone]), f"{what}: ids differ for query {i}"
            assert sorted(got.ids[i, :c].tolist()) == sorted(ref.ids[i, :c].tolist()), f"{what}: id sets differ for query {i}"
        return
    bad = np.nonzero((got.ids != ref.ids).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8]}: {got.ids[bad[0]][:8]} expected {ref.ids[bad[0]][:8]}"
    by_bits = kind.mode != "topk" or any(o[0] == "numeric_variant" for o in kind.opts)
    if by_bits:
        bad = np.nonzero(((bits(got.scores) != bits(ref.scores)) & valid).any(axis=1))[0]
        assert bad.size == 0, f"{what}: score bits differ for queries {bad[:8]}"
    else:
        np.testing.assert_allclose(got.scores[valid], ref.scores[valid], rtol=RTOL, atol=0, err_msg=what)


def _check_posting(kind, got, ref, what):
    """tests/test_gpu_parity.py::_mstg_compare: counts and distances exactly (the sign of a zero apart), ids wherever the distance is
    unique, a tie at the cut resolved among the oracle's candidates at that distance"""
    xi, xs, xc = ref.probed
    osc, oids, top_k = ref.scores, ref.ids, ref.top_k
    assert np.array_equal(got.counts, ref.counts), f"{what}: counts differ"
    _padding(kind, got, ref.counts.astype(np.int64), what)
    for i in range(len(ref.counts)):
        c = int(ref.counts[i])
        if c == 0:
            continue
        sc, ids = got.scores[i], got.ids[i]
        assert np.array_equal(bits(xs[i, :c]), bits(osc[i, :c]))
        assert np.array_equal(bits(sc[:c]) & 0x7fffffff, bits(osc[i, :c]) & 0x7fffffff), f"{what}: distances differ for query {i}"
        assert (np.diff(sc[:c]) >= 0).all() and (sc[:c] >= 0).all(), what
        uniq = np.ones(c, bool)
        uniq[1:] &= sc[1:c] != sc[:c - 1]
        uniq[:-1] &= sc[:c - 1] != sc[1:c]
        n_x = int(xc[i])
        cut_tie = n_x > c and xs[i, c] == osc[i, c - 1]
        if cut_tie:
            assert n_x < top_k + 64 or xs[i, n_x - 1] != osc[i, c - 1], "tie group longer than the look-ahead"
            uniq &= sc[:c] != osc[i, c - 1]
        assert np.array_equal(ids[:c][uniq], oids[i, :c][uniq]), f"{what}: ids differ for query {i}"
        if not cut_tie:
            assert sorted(ids[:c].tolist()) == sorted(oids[i, :c].tolist()), f"{what}: id sets differ for query {i}"
        else:
            d = osc[i, c - 1]
            lo_g, lo_o = sc[:c] != d, osc[i, :c] != d
            assert sorted(ids[:c][lo_g].tolist()) == sorted(oids[i, :c][lo_o].tolist())
            pool = set(xi[i, :n_x][xs[i, :n_x] == d].tolist())
            tied = ids[:c][~lo_g].tolist()
            assert len(tied) == int((~lo_o).sum()) and len(set(tied)) == len(tied) and set(tied) <= pool


def as_result(ref):
    """a reference as the Result the library would return for it (the host test runs `check` on it: the rule accepts its own reference)"""
    return Result(ref.ids.copy(), ref.scores.copy(), ref.counts.copy(), None if ref.diag is None else ref.diag.copy())
