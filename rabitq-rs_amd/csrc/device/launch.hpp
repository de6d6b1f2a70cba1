// launch.hpp — host-callable launchers of the kernel translation units.  The api_*.hip units (pure host code) see the
// kernels only through these; each .hip file below compiles on its own, so a change to the host side does not
// rebuild k_scan's instantiations and vice versa.
//   k_query.hip  k_prep / k_prep_wave, k_rank_* , k_select*, k_probes_given     (kernels.hpp, rank_mfma.hpp, canon_score.hpp, select_*.hpp)
//   k_scan.hip   k_scan<DT, EX, TR>                                               (scan.hpp, scan_codes.hpp, topk.hpp)
//   k_range.hip  k_range<DT, EX>: the range search's scan against a constant radius     (range.hpp, scan_codes.hpp)
//   k_range_exact.hip  k_range<0, 0, V, XR, XIP>: the same scan, its matches decided by the raw rows  (range.hpp, rerank_score.hpp)
//   k_build.hip  encoder, reference-layout -> device-layout converters, sorting   (encode.hpp)
//   k_gemm_shortlist.hip  the front of the GEMM-shortlist paths (finite check, norms, split images, dots), KmGemmAssign (km_common.hpp)
//   k_kmeans.hip Faiss-style k-means (run_kmeans_with_config) and its host driver         (km_common.hpp)
//   k_hcluster.hip  MSTG hierarchical balanced k-means and its host driver                (km_common.hpp)
//   k_save.hip   RBQ1 writer: device layout -> save_to_writer's cluster bytes, CRC-32 on the GPU
//   k_fetch.hip  fetch_embedding: id map, decode + inverse rotation of stored vectors
//   k_bf.hip     brute-force index: distances and the BinaryHeap replay                  (bf.hpp, topk.hpp)
//   k_bf_train.hip  brute-force index: the encoder's flat output, ex_code_packed         (encode_vec.hpp)
//   k_mstg.hip   MSTG closure assignment (ClosureAssigner::assign) and its host driver       (km_common.hpp)
//   k_mstg_save.hip  `.mstg` writer and loader: device layout <-> the crate's bincode records
//   k_load.hip   streamed RBQ1 loader: spans of the stream -> device layout, ex-code prefix check
//   k_mstg_search.hip  MSTG search: exact nearest centroids and dynamic_prune               (km_common.hpp, canon_score.hpp)
//   k_mstg_refine.hip  refined MSTG search: ex-code distances of a candidate pool, unique ids (kernels.hpp, scan_codes.hpp, mstg_pool.hpp)
//   k_mstg_rerank.hip  exact rerank of the MSTG pool: one entry per id, exact scores from the raw rows (mstg_pool.hpp, rerank_score.hpp)
//   k_rerank_pool.hip  pooled rerank: exact scores of a candidate pool from whole lines of the raw rows, order in LDS (rerank_score.hpp)
//   k_append.hip rbq_index_append: carry of an index into a larger geometry, id bound, nearest list of rotated rows (km_common.hpp)
//   k_remove.hip rbq_index_remove_ids: keep masks against a sorted id set, slot map, gather of an index into a smaller geometry
#pragma once
#include <atomic>
#include <string>

#include "types.hpp"

namespace rbq_host { struct HcResult; } // csrc/host/rbq_hcluster.hpp
namespace rbq_host { struct LoadPiece; } // csrc/host/rbq_load_stream.hpp

namespace rbq {

// Raises a kernel's dynamic-LDS limit once per (kernel, device, size): hipFuncSetAttribute is slow and serialises
// launches, so the largest value set so far is remembered per device.  The limit is only ever RAISED, and the check-and-set
// is serialised: two caller threads that need different sizes cannot leave the kernel with the smaller one.
struct LdsAttrCache {
    std::atomic<size_t> set[16];
    LdsAttrCache() { for (auto& v : set) v.store(0, std::memory_order_relaxed); }
    hipError_t ensure(const void* fn, size_t lds, int device);
};

// Launch probe (diagnostic: rbq_debug_stage_resources).  While the calling thread has a probe installed, the four stage
// launchers record WHICH kernel instantiation they would launch, and its geometry, instead of launching it.
struct KernelProbe { const void* fn = nullptr; uint32_t grid_x = 0, grid_y = 0, grid_z = 0, block = 0; size_t dyn_lds = 0;
                     uint32_t operands = 0; }; // (rank stage) what the GEMM multiplies: kRankOps*
constexpr uint32_t kRankOpsBf16x3 = 1, kRankOpsF16 = 2, kRankOpsF32 = 3;
struct StageProbes { KernelProbe k[4]; }; // prep, rank, select, scan
StageProbes*& stage_probes(); // this thread's probe (null: launch normally)
inline bool probe_stage(int stage, const void* fn, dim3 grid, uint32_t block, size_t lds, uint32_t operands = 0) {
    StageProbes* p = stage_probes();
    if (!p) return false;
    p->k[stage].operands = operands;
    p->k[stage].fn = fn; p->k[stage].grid_x = grid.x; p->k[stage].grid_y = grid.y; p->k[stage].grid_z = grid.z;
    p->k[stage].block = block; p->k[stage].dyn_lds = lds;
    return true;
}

struct PrepParams {
    const void* queries;  // [nq][dim] elements of query_dtype
    uint32_t nq, dim, D, Dc;
    int rotator;
    int query_dtype = kRawF32; // kRawF32 / kRawF16 / kRawBf16: picks the instantiation of the preparation kernel (host side only)
    const uint8_t* rot_blob;
    uint32_t trunc;
    float fac;
    uint32_t ex_bits;
    float* rot;          // [nq][D]
    uint8_t* lut;        // [nq][4Dc]
    QueryConsts* consts; // [nq]
    uint16_t* rot_hl;    // split-bf16 image [nq][2 D] (hi | lo per K slab, hl_layout.hpp) or null
    float* rank_resid = nullptr; // non-null (the one-product f16 route): rot_hl receives the f16 image [nq][D] instead and
                                 // rank_resid[q] = |q - f16(q)|, rounded up
    bool wg_prep;        // one workgroup per query (always for the matrix rotator)
};
hipError_t launch_prep(const PrepParams& p, int device, hipStream_t s);

struct RankParams {
    int metric;
    const float* rot;
    const uint16_t *rot_hi, *rot_lo;
    const float* cent;
    const uint16_t *cent_hi, *cent_lo;
    // the split-bf16 operands: two planes [rows][D] each, or (rot_hl / cent_hl) ONE image [rows][2 D] at *_hi with hi | lo interleaved
    // per K slab (hl_layout.hpp), *_lo unused
    bool rot_hl = false, cent_hl = false;
    const QueryConsts* consts;
    const float* cnorm2;
    uint32_t nq, nlist, D;
    float* scores; // [nq][nlist]
    bool split;    // split-bf16 MFMA GEMM (else f32 MFMA)
    bool big;      // 128x128 tiles
    bool wide;     // 128x256 tiles (split-bf16 only): problems of at least 2048 such tiles
    bool f16 = false; // one-product f16 GEMM (k_rank_f16_db): rot_hi / cent_hi are the f16 images [rows][D]; needs split, ksplit <= 1
    uint32_t ksplit = 0; // > 1: split-K over grid.z (split-bf16, 64 / 128 tiles): parts added atomically to a row the preparation zeroed
};
hipError_t launch_rank_exact(const RankParams& p, hipStream_t s);
hipError_t launch_rank_gemm(const RankParams& p, int device, hipStream_t s);
// latency-first front of a small call (latency.hpp): prep + the exact canonical score of every list in ONE launch (FhtKac / no rotator)
hipError_t launch_lat_front(const PrepParams& p, const RankParams& r, int device, hipStream_t s);

constexpr uint32_t kAuditCap = 1023; // dead lists exported per query under lazy_audit (a shortlist holds fewer)
// words per query of the head-bound tap (option ub_tap): ncand, h, g_add / g_err bits of the 4 head lists, 256 x (gblock, U bits, nvalid)
constexpr uint32_t kHeadUbRow = 2 + 8 + 3 * 256;
struct SelectParams {
    float* scores;
    uint32_t nq, nlist, nprobe;
    int metric;
    const float* rot;
    const float* cent;
    uint32_t D;
    const QueryConsts* consts;
    float cnorm2_max;
    const float* rank_resid = nullptr; // non-null: the scores come from the one-product f16 GEMM — [nq] |q - f16(q)|, and
    float cnorm_max = 0.0f, rc_max = 0.0f; // sqrt(cnorm2_max) and the largest |c - f16(c)|, both rounded up (eps: rank_mfma.hpp header)
    const uint32_t *list_gb0, *list_n;
    ProbeInfo* probe;
    StreamItem* wl;
    uint64_t wl_stride;
    uint32_t* nstream;
    unsigned long long* nvec;
    unsigned long long* prof_total; // null unless a profile is open: slot kProfVectorsProbed of the striped counters (types.hpp)
    unsigned int* fallback_count;
    int force_fallback;
    const BlockSummary* bsum;
    // lazy selection (k_select_mfma only): lists that are provably skipped as a whole are neither scored nor streamed
    const float* cnorm2;          // [nlist] squared centroid norms (inner-product metric: distance from the approximate dot)
    const BlockSummary* lsum;     // [nlist] factor ranges of every list
    const BlockSummaryEx* bsumx;  // [n_blocks] ex-factor ranges of every block
    uint32_t* dead_skipped;       // [4][nq] out: vectors of probed lists dropped that way (exact when exact_members, else 0) |
                                  //              number of lists that go to the scan | two diagnostics taps (T_ub bits; z0, n, scored)
    uint32_t top_k, ex_bits;
    int lazy;                     // 0: every probed list is scored and streamed (round-2 behaviour)
    int exact_members;            // diagnostics: dead_skipped and the probed-vector count must be exact
    // exact head evaluation (round 4): a select-time bound of the k-th distance from REAL estimates of the nearest list's first vectors
    const uint8_t* lut;           // [nq][4Dc] the queries' u8 LUTs (k_prep), device codebook order
    const uint8_t* blocks;        // the index's block records / ex codes / ex factors, as k_scan reads them
    const uint8_t* ex_codes;
    const float *f_add_ex, *f_rescale_ex;
    uint32_t Dc;
    uint32_t n_blocks;            // blocks of the index (the exact head evaluation checks its geometry against it)
    const uint32_t* filter;       // dense id filter of search_filtered (or null) and the ids it tests: under a filter only the exact
    uint64_t filter_nbits;        // head evaluation — which counts filter-passing vectors only — can bound the k-th distance
    const uint64_t* ids;
    int head_exact;               // 0: Cauchy-Schwarz bound only (round 3)
    SlackMul slack;               // TEST ONLY: multipliers of block_ub()'s rounding-slack terms (all 1 in the product)
    uint32_t* audit_dead;         // null, or (option lazy_audit) [nq][kAuditCap + 1] u32: the number of lists this query's selection dropped as
                                  // a whole, then their ids — exported WITHOUT changing any decision, with or without diagnostics or a
                                  // filter, so that a test can ask the oracle what the reference did with exactly those lists
    uint32_t* head_ub;            // null, or (option ub_tap) [nq][kHeadUbRow] u32: the head candidates of the lazy selection and their
                                  // bounds U (block_ub), written WITHOUT changing any decision (layout at kHeadUbRow)
    uint32_t numeric_variant;     // kVarAvx512 / kVarAvx2 / kVarPortable (kernels.hpp): picks the instantiation (host side only)
    int fault_dead_all;           // TEST ONLY (debug option lazy_fault_inject, default 0): T_ub := -inf — every list behind the head is
                                  // declared dead whatever its bounds say: a deliberately WRONG selection, so that the
                                  // bound_violations audit can be shown to catch one
};
// key_window: null, or [nq][select_exact_np2(nprobe)] u64 in global memory (nprobe > kNprobeMax: the exact path with its key
// window outside the LDS — slow, but every nprobe up to n_lists is served, as the reference does, src/ivf.rs:1791)
uint32_t select_exact_np2(uint32_t nprobe);
hipError_t launch_select_exact(const SelectParams& p, int device, hipStream_t s, uint64_t* key_window);
hipError_t launch_select_mfma(const SelectParams& p, int device, hipStream_t s);

struct ProbesGivenParams {
    const uint32_t *list_ids, *list_counts;
    uint32_t max_lists, nq, nlist;
    int metric;
    const float* rot;
    const float* cent;
    uint32_t D;
    const uint32_t *list_gb0, *list_n;
    ProbeInfo* probe;
    StreamItem* wl;
    uint64_t wl_stride;
    uint32_t* nstream;
    const QueryConsts* consts;
    const BlockSummary* bsum;
    uint32_t numeric_variant;     // kVarPortable: block_lbmin's epilogue is not fused
};
hipError_t launch_probes_given(const ProbesGivenParams& p, hipStream_t s);

// ev0/ev1: null, or an event pair carried by the dispatch packet itself (hipExtLaunchKernelGGL)
hipError_t launch_scan(const ScanParams& P, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// k_scanw (scanw.hpp): the same scan with one wave per query; scanw_serves(): the call shapes it takes (launch_scan routes
// to it when ScanParams::wave_kernel is set and it serves the call)
// k_range (range.hpp, k_range.hip): the range search's scan — the same stream against a constant threshold, matches in scan order
hipError_t launch_range(const RangeParams& P, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
// the exact range scan (k_range_exact.hip): the estimate's matches scored against their raw rows, kept by the exact score.
// hipErrorInvalidValue without raw rows (raw null or n_raw 0), for an unknown raw_dtype, or when the LDS does not fit
hipError_t launch_range_exact(const RangeExactParams& P, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);
bool scanw_serves(const ScanParams& P);
hipError_t launch_scanw(const ScanParams& P, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// ---- k_build.hip -------------------------------------------------------------------------------------------------
hipError_t launch_rotate_rows(const float* src, const uint32_t* map, uint32_t nrows, uint32_t dim, uint32_t D, int rotator,
                              const uint8_t* rot_blob, uint32_t trunc, float fac, float* rows, hipStream_t s);
hipError_t launch_encode(const EncodeParams& P, hipStream_t s);
// k_rescale.hip: best_rescale_factor of every row (one workgroup per row).  raw_o = false: rows are rotated vectors, o is
// |row - centroid of the row's list| / norm (block mode: list = block_list[r / 32]; row_slot != null: block_list[row_slot[r] / 32]);
// raw_o = true: rows are o itself (test hook).  Rows with slot_src[r] == kNoSrc are skipped.  D <= 2048, 1 <= ex_bits <= 7.
hipError_t launch_rescale(const float* rows, const float* centroids, const uint32_t* block_list, const uint32_t* row_slot,
                          const uint32_t* slot_src, uint32_t nrows, uint32_t D, uint32_t ex_bits, bool raw_o, double* t,
                          hipStream_t s);
// raw ex codes [row][D] u8 -> lane-major units of slot (row_slot ? row_slot[row] : row) in `ex`
hipError_t launch_pack_ex(const uint8_t* raw, const uint32_t* slot_src, const uint32_t* row_slot, uint32_t nrows, uint32_t D,
                          uint32_t ex_bits, uint8_t* ex, hipStream_t s);
hipError_t launch_block_summary(const uint8_t* blocks, const uint32_t* block_nv, uint32_t nblocks, uint32_t Dc, BlockSummary* bsum,
                                hipStream_t s);
// per-block Cauchy-Schwarz bound terms (BlockSummaryEx) and per-list factor ranges (lazy probe selection); one workgroup per list
hipError_t launch_list_summaries(const uint8_t* blocks, const uint8_t* ex, const float* fadd_ex, const float* fres_ex, const float* cent,
                                 const BlockSummary* bsum, const uint32_t* list_gb0, const uint32_t* list_n, uint32_t nlist, uint32_t D,
                                 uint32_t Dc, uint32_t ex_bits, BlockSummaryEx* bsumx, BlockSummary* lsum, hipStream_t s);
hipError_t launch_count_assign(const uint32_t* assign, uint64_t n, uint32_t nlist, uint32_t* counts, uint32_t* err, hipStream_t s);
hipError_t launch_iota(uint32_t* x, uint64_t n, hipStream_t s);
hipError_t launch_scatter_slots(const uint32_t* sorted_list, const uint32_t* sorted_src, uint64_t n, const uint32_t* list_gb0,
                                const uint64_t* vstart, uint32_t* slot_src, hipStream_t s);
// stable radix sort of (key, value) u32 pairs on the low `bits` bits; tmp == null returns the scratch size in *tmp_bytes
hipError_t sort_pairs_u32(void* tmp, size_t* tmp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                          uint32_t* vals_out, size_t n, unsigned bits, hipStream_t s);
// streamed build: rows of a pushed chunk sorted by (list, source index) -> first row per list, global slot per row
// (first slot of the list + vectors pushed by earlier chunks + rank in this chunk), then advance the cursors
hipError_t launch_chunk_first(const uint32_t* sorted_list, uint32_t n, uint32_t* chunk_first, hipStream_t s);
hipError_t launch_chunk_slots(const uint32_t* sorted_list, const uint32_t* sorted_src, uint32_t n, const uint32_t* list_gb0,
                              const uint32_t* list_cursor, const uint32_t* chunk_first, uint32_t* row_src, uint32_t* row_slot,
                              hipStream_t s);
hipError_t launch_chunk_advance(const uint32_t* sorted_list, uint32_t n, const uint32_t* chunk_first, uint32_t* list_cursor,
                                hipStream_t s);
// reference layout -> device layout (rbq_index_create / load_rbq1): `recs` = the reference's batch records of nb
// blocks back to back; `exsrc` = the packed ex codes of the chunk's vectors, dense, in list order; block b's first
// vector is entry block_dense0[b] of the dense arrays
hipError_t launch_relayout_blocks(const uint8_t* recs, uint32_t nb, uint32_t D, uint32_t Dc, uint8_t* blocks, hipStream_t s);
hipError_t launch_relayout_ex(const uint8_t* exsrc, const uint64_t* block_dense0, const uint32_t* block_nv,
                              uint32_t nb, uint32_t D, uint32_t ex_bits, uint8_t* ex, hipStream_t s);
// per-slot arrays from per-vector (dense, list order) arrays: dst[b*32+v] = v < nv[b] ? src[dense0[b]+v] : fill
hipError_t launch_spread_u64(const uint64_t* src, const uint64_t* block_dense0, const uint32_t* block_nv, uint32_t nb, uint64_t fill,
                             uint64_t* dst, hipStream_t s);
hipError_t launch_spread_f32(const float* src, const uint64_t* block_dense0, const uint32_t* block_nv, uint32_t nb, float fill,
                             float* dst, hipStream_t s);
// centroid-derived arrays: squared norms (f64 accumulate, as the host did) and the split-bf16 image
hipError_t launch_centroid_arrays(const float* cent, uint32_t nlist, uint32_t D, float* cnorm2, uint16_t* hl, hipStream_t s);
// the one-product f16 image [nlist][D] of the centroids and |c - f16(c)| per centroid, rounded up (relayout.hpp)
hipError_t launch_centroid_f16(const float* cent, uint32_t nlist, uint32_t D, uint16_t* img, float* resid, hipStream_t s);
// the planar hi / lo planes [rows][D] of an interleaved split-bf16 image [rows][2 D] (hl_layout.hpp): debug option rank_planar
hipError_t launch_hl_planes(const uint16_t* hl, uint64_t rows, uint32_t D, uint16_t* hi, uint16_t* lo, hipStream_t s);
// (kRawF32 / kRawF16 / kRawBf16, the element types of the raw rows and of the query rows: types.hpp)
// exact re-scoring of the returned ids against caller-supplied raw vectors (optional rerank, default off)
// (queries: [nq][dim] elements of query_dtype, widened as they are copied into LDS)
hipError_t launch_rerank(const void* queries, int query_dtype, uint32_t nq, uint32_t dim, const void* raw, int raw_dtype, uint64_t n_raw, int metric,
                         uint32_t top_k, uint64_t* ids, float* scores, const uint32_t* counts, hipStream_t s);
// pooled rerank (option rerank_pool; k_rerank_pool.hip): the exact scores of a query's pool of candidates
// (the result of the search at top_k := pool), ordered by (exact score, rank in the pool); the first top_k are the answer
constexpr uint32_t kRerankPoolMax = 4096; // one workgroup orders a query's pool in LDS (the figure of kMrPoolMax, for its reason)
struct RerankPoolParams {
    const void* queries;         // [nq][dim] elements of query_dtype, input space
    const void* raw;             // [n_raw][dim] elements of raw_dtype
    uint64_t n_raw;
    uint32_t nq, dim, metric;
    uint32_t pool, top_k;        // top_k < pool <= kRerankPoolMax
    const uint64_t* pool_ids;    // [nq][pool]
    const uint32_t* pool_counts; // [nq]
    uint64_t* out_ids;           // [nq][top_k]
    float* out_scores;           // [nq][top_k]
    uint32_t* out_counts;        // [nq]
    int raw_dtype = kRawF32;     // kRawF32 / kRawF16 / kRawBf16
    int query_dtype = kRawF32;   // the same values: what `queries` holds
    uint32_t raw_by_element = 0; // set by the launch: 16-bit rows that do not all start 4-byte aligned (odd dim, or raw at 2 mod 4)
};
size_t rerank_pool_lds_bytes(uint32_t dim, uint32_t pool);
hipError_t launch_rerank_pool(const RerankPoolParams& P, int device, hipStream_t s);

// brute-force index (bf.hpp, k_bf.hip): distances of a (query sub-batch x vector chunk), then the per-query BinaryHeap replay
struct BfDistParams {
    const float* rot;          // [nq][D] rotated queries (k_prep)
    const QueryConsts* consts; // [nq]
    uint32_t nq, D, ex_bits;
    uint64_t v0, nv;           // the chunk: vector ids v0 .. v0 + nv - 1
    const uint8_t* bin;        // [n][D/8]
    const uint8_t* ex;         // [n][D*ex_bits/8]
    const float *f_add, *f_rescale, *f_add_ex, *f_rescale_ex; // [n]
    const uint32_t* filter;    // dense id bitset or null
    uint64_t filter_nbits;
    float* dist;               // [nq][nv]
};
hipError_t launch_bf_dist(const BfDistParams& p, hipStream_t s);
struct BfSelectParams {
    const float* dist;         // [nq][nv]
    uint32_t nq, top_k;
    uint64_t v0, nv;
    int metric;
    int first, last;           // first / last vector chunk of the call
    bool lds_heap;             // the heap lives in LDS during the launch (else in heap_d / heap_s)
    float* heap_d;             // [nq][top_k + 1]: the heap between chunks (and during them when !lds_heap)
    uint32_t* heap_s;
    uint32_t* heap_len;        // [nq]
    uint64_t* out_ids;         // [nq][top_k]
    float* out_scores;
    uint32_t* out_counts;      // [nq]
    unsigned long long* stats; // [2]: heap pushes, pushes decided by a tie (rbq_bf_debug_heap_stats)
};
hipError_t launch_bf_select(const BfSelectParams& p, hipStream_t s);
constexpr uint32_t kBfLdsHeapMaxTopK = 8191; // (top_k + 1) * 8 bytes of LDS heap <= 64 KiB
// k_bf_train.hip: BruteForceRabitqIndex::train.  launch_bf_encode: k_encode's flat mode over P.nslots rotated rows (see
// EncodeParams; P.t_row != null: the per-vector rescale factors of launch_rescale).  launch_bf_pack_ex: raw ex codes [nrows][D]
// u8 -> the crate's ex_code_packed [nrows][D * ex_bits / 8] (ex_bits 2 or 6)
hipError_t launch_bf_encode(const EncodeParams& P, hipStream_t s);
hipError_t launch_bf_pack_ex(const uint8_t* raw, uint64_t nrows, uint32_t D, uint32_t ex_bits, uint8_t* ex, hipStream_t s);

// ---- the GEMM-shortlist front (k_gemm_shortlist.hip): what k-means, hierarchical clustering, the MSTG closure assignment and the
// MSTG list selection do before their own scan and exact kernels.  Non-owning: every buffer is the caller's.
inline uint32_t km_dp(uint32_t dim) { return (dim + 31u) / 32u * 32u; } // the padded dimension of the split images
// workspace bytes per row of a chunk: scores (4k), split image (4 Dp), shortlist of `cap` entries and its length
inline uint64_t gemm_shortlist_row_bytes(uint64_t k, uint32_t Dp, uint32_t cap) { return 4 * k + 4ull * Dp + 4ull * cap + 4; }
struct CentView {          // prepared centroids
    uint32_t k, dim, Dp;
    float* nc;             // [k] canonical norms
    uint32_t* ncmax_bits;  // their maximum (bit pattern of a non-negative float)
    uint16_t *hi, *lo;     // [k][Dp] split-bf16 planes, zero beyond dim (launch_centroid_norms: unused)
};
hipError_t launch_centroid_norms(const float* cent, const CentView& v, hipStream_t s);  // nc and ncmax_bits
hipError_t launch_split_centroids(const float* cent, const CentView& v, hipStream_t s); // the same, then hi / lo
// *bad = x[0, count) holds a non-finite value; d_flag is one device word of scratch; returns once the answer is known
hipError_t nonfinite_sync(const float* x, uint64_t count, uint32_t* d_flag, hipStream_t s, bool* bad);
hipError_t launch_row_norms(const float* x, uint64_t rows, uint32_t dim, float* out, hipStream_t s); // canonical norms of x [rows][dim]
// dots = approximate inner products of rows [0, nr) of x with the centroids: the ranking GEMM's inner-product form over the rows' split
// image in xh / xl.  xh, xl [nr rounded up to 128][Dp], dots [nr rounded up to 128][k]; image rows beyond nr are stale, their scores unused.
hipError_t launch_approx_dots(const float* x, uint32_t nr, uint32_t dim, const CentView& v, uint16_t* xh, uint16_t* xl, float* dots,
                              int device, hipStream_t s);
// TEST ONLY (rbq_debug_gemm_shortlist_front, include/rbq_kmeans.h): the front alone over HOST rows and centroids, in passes of
// km_chunk_rows rows, through the launchers above and nothing else; every pointer is the caller's host memory
struct FrontTapArgs {
    const float* centroids; // [k][dim]
    uint64_t k;
    uint32_t dim;
    const float* rows;      // [n][dim]
    uint64_t n;
    float *dots, *nx, *nc, *ncmax;                  // [n][k], [n], [k], [1]
    uint16_t *row_hi, *row_lo, *cent_hi, *cent_lo;  // [n][Dp] / [k][Dp], each pair null or given
};
int gemm_shortlist_front_tap(const FrontTapArgs& a, int device, std::string& detail); // RBQ_* code; detail on failure

// ---- k-means (k_kmeans.hip): run_kmeans_with_config on the current device, arguments already validated (rbq_kmeans_device)
constexpr uint64_t kKmeansChunkBytes = 512ull << 20; // per-chunk assignment workspace (R rows x gemm_shortlist_row_bytes, R >= 128)
// test hooks of KmGemmAssign (km_common.hpp), defined in k_gemm_shortlist.hip: a cap on the rows per pass
// (rbq_debug_set_kmeans_chunk_rows, 0: none) and the passes run so far (rbq_debug_kmeans_assign_passes)
extern std::atomic<uint64_t> g_km_chunk_rows_cap, g_km_assign_passes;
struct KMeansArgs {
    const float* data; // device [n][dim]
    uint64_t n;
    uint32_t dim;
    uint64_t k, niter, nredo, seed;
    int spherical;
    uint64_t mppc, dbs;
    int device;
    float* centroids;       // host [k][dim]
    uint32_t* assignments;  // device [n]
    double* objective;      // host
    uint64_t* stats;        // host [4] or null: shortlist fallbacks, empty clusters reseeded, RNG draws, largest shortlist
};
int kmeans_device(const KMeansArgs& a, std::string& detail); // RBQ_* code; detail on failure

// ---- MSTG closure assignment (k_mstg.hip): ClosureAssigner::assign of every row, arguments already validated
constexpr uint32_t kMstgMaxReplicas = 64;
struct ClosureArgs {
    const float* centroids; // [k][dim], host or device (cent_on_device)
    uint64_t k;
    uint32_t dim;
    const float* data;      // [n][dim], host or device (data_on_device)
    uint64_t n;
    float epsilon;
    uint32_t max_replicas;
    uint64_t max_chunk_rows; // 0 = by the workspace budget
    bool cent_on_device, data_on_device, out_on_device;
    uint32_t* out_lists;    // [n][max_replicas] (unused slots UINT32_MAX) and [n]; null with a tap
    uint32_t* out_counts;
    uint32_t* tap_sl;       // host, null or [n][kShortlist] / [n]: the shortlists only (rbq_mstg_debug_closure_shortlist)
    uint32_t* tap_sl_n;
    uint64_t* fallbacks;    // host out: rows scored against every centroid
};
int closure_device(const ClosureArgs& a, int device, std::string& detail); // RBQ_* code; detail on failure
// (vector, list) pairs of the closure in vector-major order: pair off[i] + j = (i, lists[i][j]) for j < counts[i]
hipError_t launch_closure_expand(const uint32_t* lists, const uint32_t* counts, const uint32_t* off, uint64_t n, uint32_t max_replicas,
                                 uint32_t* pair_list, uint32_t* pair_vec, hipStream_t s);

// ---- MSTG hierarchical balanced clustering (k_hcluster.hip): HierarchicalClustering::cluster, arguments already validated
struct HClusterArgs {
    const float* d_data;  // device [n][dim]
    const float* h_data;  // the same rows in host memory, or null (rows handed to the host are then copied back)
    uint64_t n;
    uint32_t dim;
    uint64_t max_size, k, niter;
    float balance_weight;
    uint64_t host_below;  // a cluster of at most this many rows goes to the host with its subtree; 0 = never
    int device;
};
int hcluster_device(const HClusterArgs& a, rbq_host::HcResult& out, std::string& detail); // RBQ_* code; detail on failure

// ---- MSTG search (k_mstg_search.hip): the exact ef_search nearest centroids of every query and dynamic_prune's cut
constexpr uint32_t kMsCap = 2048; // shortlist capacity per query (the exact pass sorts it in LDS)
struct MstgSelectParams {
    const float* rot;       // [nq][cv.dim] the queries as k_prep leaves them (rotator NONE: the raw query)
    uint32_t nq;
    uint32_t ef_search;
    float pruning_epsilon;
    const float* cent;      // [cv.k][cv.dim]
    CentView cv;            // k, dim, Dp always; the GEMM path (mstg_select_gemm): as launch_split_centroids left it
    uint32_t cent_bad;      // a centroid coordinate is not finite: every query is scored against every centroid
    // per-chunk scratch of the GEMM path
    uint16_t *q_hi, *q_lo;  // [nq rounded up to 128][Dp]
    float* nx;              // [nq]
    float* dots;            // [nq rounded up to 128][k]
    uint32_t* sl;           // [nq][kMsCap]
    uint32_t* sl_n;         // [nq] (k > 256)
    unsigned long long* keys_g; // [nq][mstg_select_knp2(k)] (k > kMsCap), else null
    unsigned long long* fallbacks; // device counter: queries scored against every centroid
    uint32_t* out_lists;    // [nq][min(ef_search, k)] in scan order, unused slots UINT32_MAX
    uint32_t* out_counts;   // [nq]
};
bool mstg_select_gemm(uint64_t k, uint32_t D);  // whether this shape takes the GEMM shortlist
uint32_t mstg_select_knp2(uint64_t k);          // keys per query of keys_g (0: not needed)
hipError_t launch_mstg_select(const MstgSelectParams& p, int device, hipStream_t s);

// ---- refined MSTG search (k_mstg_refine.hip): the binary scan's pool re-scored with the ex codes, one entry per id, top_k
constexpr uint32_t kMrPoolMax = 4096; // RBQ_MSTG_REFINE_POOL_MAX: the pool of one query is sorted in LDS
struct MstgRefineParams {
    const uint8_t* blocks;      // the index, as ScanParams names it
    const uint64_t* ids;
    const uint8_t* ex_codes;
    const float *f_add_ex, *f_rescale_ex;
    const uint32_t* blk_list;   // [n_blocks] the list of every block (launch_mstg_refine_maps)
    uint64_t n_slots;           // n_blocks * 32
    const uint8_t* lut;         // [nq][4Dc], rot [nq][D], consts [nq]: as k_prep left them (with the handle's ex_bits)
    const float* rot;
    const QueryConsts* consts;
    const ProbeInfo* probe;     // [nq][probe_stride] as k_probes_given wrote them; list_counts [nq] rows in use
    const uint32_t* list_counts;
    uint32_t probe_stride;
    const uint64_t* pool_slots; // [nq][pool] the binary scan's result over the identity slot map, pool_scores [nq][pool] its
    const float* pool_scores;   // estimates (ascending), pool_counts [nq]
    const uint32_t* pool_counts;
    uint32_t pool, pool_np2;    // pool_np2: the power of two >= pool (<= kMrPoolMax)
    uint64_t* out_ids;          // [nq][top_k], out_scores [nq][top_k], out_counts [nq]
    float* out_scores;
    uint32_t* out_counts;
    uint32_t nq, D, Dc, ex_bits, metric, top_k, numeric_variant;
};
size_t mstg_refine_lds_bytes(uint32_t D, uint32_t Dc, uint32_t ex_bits, uint32_t pool_np2);
// slot_map [n_blocks * 32] u64 = the identity; blk_list [n_blocks] u32
hipError_t launch_mstg_refine_maps(const uint32_t* list_gb0, const uint32_t* list_n, uint32_t n_lists, uint32_t n_blocks, uint64_t* slot_map,
                                   uint32_t* blk_list, hipStream_t s);
hipError_t launch_mstg_refine(const MstgRefineParams& P, int device, hipStream_t s);

// ---- exact rerank of the MSTG pool (option mstg_rerank; k_mstg_rerank.hip): the same pool, one entry per
// id, each distinct id scored exactly against its raw row, ordered by (distance, rank), top_k.  The distance is canon_l2 or -canon_dot.
struct MstgRerankParams {
    const uint64_t* ids;        // the index's ids in slot order
    const uint32_t* blk_list;   // [n_blocks] the list of every block (launch_mstg_refine_maps)
    uint64_t n_slots;           // n_blocks * 32
    const ProbeInfo* probe;     // [nq][probe_stride] as k_probes_given wrote them; list_counts [nq] rows in use
    const uint32_t* list_counts;
    uint32_t probe_stride;
    const uint64_t* pool_slots; // [nq][pool] the binary scan's result over the identity slot map, pool_scores [nq][pool] its
    const float* pool_scores;   // estimates (ascending), pool_counts [nq]
    const uint32_t* pool_counts;
    uint32_t pool, pool_np2;    // pool_np2: the power of two >= pool (<= kMrPoolMax); top_k <= pool
    const void* queries;        // [nq][dim] elements of query_dtype, input space (the caller's rows)
    const void* raw;            // [n_raw][dim] elements of raw_dtype, n_raw >= 1
    uint64_t n_raw;
    uint64_t* out_ids;          // [nq][top_k], out_scores [nq][top_k], out_counts [nq]
    float* out_scores;
    uint32_t* out_counts;
    uint32_t nq, dim, metric, top_k;
    int raw_dtype = kRawF32;     // kRawF32 / kRawF16 / kRawBf16
    int query_dtype = kRawF32;   // the same values: what `queries` holds
    uint32_t raw_by_element = 0; // set by the launch: 16-bit rows that do not all start 4-byte aligned (odd dim, or raw at 2 mod 4)
};
size_t mstg_rerank_lds_bytes(uint32_t dim, uint32_t pool_np2);
hipError_t launch_mstg_rerank(const MstgRerankParams& P, int device, hipStream_t s);

// ---- RBQ1 writer (k_save.hip): words [w0, w0 + nw) of the cluster section of the stream, into out[0, nw)
struct SaveParams {
    const uint64_t* woff;     // [n_lists + 1] first word of every cluster within the cluster section
    const uint32_t* list_gb0; // [n_lists] first block of every list
    const uint32_t* list_n;   // [n_lists]
    const float* centroids;   // [n_lists][D] rotated
    const uint8_t* blocks;    // device block records (stride Dc * 4 + 384)
    const uint64_t* ids;      // slot order
    const uint8_t* ex;        // lane-major ex codes, exd bytes per slot (ex_bits > 0)
    const float *fadd_ex, *fres_ex, *delta, *vl; // slot order (fadd_ex / fres_ex unused when ex_bits == 0)
    uint64_t exd;
    uint32_t n_lists, D, Dc, ex_bits, ex_words, cpu; // ex_words = D * ex_bits / 32; cpu = ex_cpu(ex_bits)
};
hipError_t launch_save_fill(const SaveParams& P, uint64_t w0, uint64_t nw, uint32_t* out, hipStream_t s);
// CRC-32/IEEE of device bytes p[0, n) (any alignment) into *out (device); seg_scratch holds crc_scratch_words(n) u32
constexpr uint32_t kCrcSegment = 4096;
uint64_t crc_scratch_words(uint64_t n);
hipError_t launch_crc32(const uint8_t* p, uint64_t n, uint32_t* seg_scratch, uint32_t* out, hipStream_t s);

// ---- `.mstg` writer and loader (k_mstg_save.hip; include/rbq_mstg_persist.h, csrc/host/rbq_mstg_file.hpp) ------------------------
// The posting-list section of the stream: list c starts (with its u64 length prefix) at section byte loff[c]; loff[n_lists] is
// the section's length.  R = bytes of one record, E = bytes of its ex_code_packed.
struct MstgSaveParams {
    const uint64_t* loff;     // [n_lists + 1]
    const uint32_t* list_gb0; // [n_lists] first block of every list
    const uint32_t* list_n;   // [n_lists]
    const float* centroids;   // [n_lists][D]
    const uint8_t* blocks;    // device block records (stride Dc * 4 + 384)
    const uint64_t* ids;      // slot order
    const uint8_t* ex;        // lane-major ex codes, exd bytes per slot (ex_bits > 0)
    const float *fadd_ex, *fres_ex, *delta, *vl, *rnorm; // slot order (fadd_ex / fres_ex unused when ex_bits == 0)
    uint64_t exd;
    uint32_t n_lists, D, Dc, ex_bits, cpu, has_t, t_bits, R, E; // (has_t, t_bits): the non-empty lists' RabitqConfig::t_const
};
// section bytes [b0, b0 + nb) into out[0, nb) (out: 4-byte aligned, room for nb rounded up to 4; b0 and nb are arbitrary)
hipError_t launch_mstg_save_fill(const MstgSaveParams& P, uint64_t b0, uint64_t nb, uint32_t* out, hipStream_t s);
// A span of the stream (bytes [span_off, ...) at `span`, any alignment inside) that holds every record of blocks
// gb_first .. gb_first + nb - 1: block b's first record lies at stream offset boff[b].  One workgroup per block writes the
// device layout of its 32 slots (pad slots as the encoder leaves them) and ORs what its records get wrong (kMstgBad*) into *err.
struct MstgLoadParams {
    const uint8_t* span;
    uint64_t span_off;
    const uint64_t* boff;       // [n_blocks]
    const uint32_t* block_nv;   // [n_blocks] real vectors of every block (1..32)
    uint32_t gb_first, nb;
    uint8_t* blocks;
    uint64_t* ids;
    uint8_t* ex;
    float *fadd_ex, *fres_ex, *delta, *vl, *rnorm;
    uint32_t* err;
    uint32_t D, Dc, ex_bits, R, E;
};
hipError_t launch_mstg_load_scatter(const MstgLoadParams& P, hipStream_t s);

// ---- streamed RBQ1 loader (k_load.hip; rbq_index_load_rbq1_stream, csrc/host/rbq_load_stream.hpp) -------------------------------
// One span of the stream's cluster region (file bytes [span_off, ...) at `span`, 256-byte aligned) and its pieces.  Workgroup w
// serves the piece with the largest wg0 <= w: it writes that piece's units into the device layout (scatter != 0: centroids,
// un-interleaved batch records, ids / factors over the 32-padded slots with their fills, re-packed ex codes) and folds the file
// position of every ex-code length prefix that is not exb into *bad_prefix with an atomic minimum.  scatter == 0: the prefix check
// only (a stream this build cannot serve, or one whose framing already failed); the output arrays are then not touched.
struct LoadSpanParams {
    const uint8_t* span;
    uint64_t span_off;
    const rbq_host::LoadPiece* pieces;
    uint32_t n_pieces, scatter;
    uint32_t D, Dc, ex_bits;
    uint64_t exb;               // bytes of a packed ex code in the stream (D * ex_bits / 8)
    uint32_t* centroids;        // [n_lists][D] f32 bit patterns
    uint8_t* blocks;
    uint64_t* ids;
    uint8_t* ex;
    uint32_t *fadd_ex, *fres_ex, *delta, *vl; // f32 bit patterns, slot order
    unsigned long long* bad_prefix;
};
hipError_t launch_load_span(const LoadSpanParams& P, uint64_t n_workgroups, hipStream_t s);
// block_nv[b] = real vectors of global block b (1..32), from the lists' first blocks and sizes
hipError_t launch_load_block_nv(const uint32_t* list_gb0, const uint32_t* list_n, uint32_t n_lists, uint32_t* block_nv, hipStream_t s);

// The per-slot arrays of a replica as the carry and the gather kernel move them from an old index (src) into a new one (dst)
struct SlotArrays {
    uint8_t *blocks, *ex;             // ex: null for a 1-bit index
    uint64_t* ids;
    float *fadd, *fres, *delta, *vl;  // fadd / fres: null for a 1-bit index
    float* rnorm;                     // MSTG handles (rbq_mstg_append, rbq_mstg_remove_ids): residual norms, a sixth per-slot array; null: none
};

// ---- rbq_index_append (k_append.hip; csrc/host/rbq_append_plan.hpp) ------------------------------------
// The arrays of an index moved into the geometry of a grown one: new block b of list c = block_list[b] takes old block
// append_src_block(b, gb0_new[c], gb0_old[c], n_old[c]) — its record, ids, ex codes, ex factors and reconstruction factors — or,
// where the list had no such block, what the streamed builder's zero fill leaves: zeros, and ids of all ones.
struct AppendCarryParams {
    const uint32_t* block_list;                 // [nb_new] list of every block of the grown index
    const uint32_t *gb0_new, *gb0_old, *n_old;  // [n_lists]
    uint32_t nb_new, nb_old;
    uint32_t rec16, ex16;                       // 16-byte units of a block record / of a block's 32 ex codes (0: 1-bit index)
    SlotArrays src, dst;
};
hipError_t launch_append_carry(const AppendCarryParams& P, int device, hipStream_t s);
// *out (device, zeroed by the caller) = max over the real slots of id + 1 (saturating); block_nv [n_blocks] as launch_load_block_nv leaves it
hipError_t launch_append_id_bound(const uint64_t* ids, const uint32_t* block_nv, uint64_t n_blocks, unsigned long long* out, hipStream_t s);
// Nearest list of rotated rows by DESIGN.md section 11's canonical distance: KmGemmAssign over rows [.][D] against cent [k][D].
struct AppendAssign; // workspace for up to `rows` rows per run
hipError_t append_assign_create(uint64_t rows, uint64_t k, uint32_t D, int device, AppendAssign** out);
hipError_t append_assign_run(AppendAssign* a, const float* rows, uint32_t n, const float* cent, uint32_t* out, hipStream_t s);
void append_assign_free(AppendAssign* a);

// ---- rbq_index_remove_ids (k_remove.hip; csrc/host/rbq_remove_plan.hpp) -------------------------------
// rocprim's radix sort of u64 keys; tmp == null returns the scratch size in *tmp_bytes
hipError_t sort_keys_u64(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, size_t n, hipStream_t s);
// mask[b] bit v = slot v of block b is real (v < block_nv[b]) and its id is not in `set` ([n_set] u64, ascending)
hipError_t launch_remove_mark(const uint64_t* ids, const uint32_t* block_nv, uint64_t n_blocks, const uint64_t* set, uint64_t n_set,
                              uint32_t* mask, hipStream_t s);
// scan[i] = kept slots (set mask bits) of blocks [0, i), i < n; tmp == null returns the scratch size in *tmp_bytes
hipError_t remove_scan_kept(void* tmp, size_t* tmp_bytes, const uint32_t* mask, uint32_t* scan, uint64_t n, hipStream_t s);
// kept[c] = kept slots of list c; scan [n_blocks + 1] as remove_scan_kept leaves it
hipError_t launch_remove_list_kept(const uint32_t* scan, const uint32_t* gb0_old, const uint32_t* n_old, uint32_t n_lists,
                                   uint64_t n_blocks, uint32_t* kept, hipStream_t s);
// map[remove_dst_slot(..)] = old slot for every kept old slot; the caller fills map [nb_new * 32] with all ones (pads) first
hipError_t launch_remove_slot_map(const uint32_t* mask, const uint32_t* scan, const uint32_t* block_list_old, const uint32_t* gb0_old,
                                  const uint32_t* gb0_new, uint64_t nb_old, uint64_t nb_new, uint32_t* map, hipStream_t s);
// The arrays of an index gathered into the geometry of a shrunk one: new slot s takes old slot map[s] — its lane of the block
// record (code granules, tail granule, factor rows), its ex code, id, ex factors and reconstruction factors — or, for a pad
// (all ones), the builder's fill: zeros, and an id of all ones.
struct RemoveGatherParams {
    const uint32_t* map;                        // [nb_new * 32] source slot of every new slot
    uint32_t nb_new, n_slots_old;
    uint32_t rec, G16, tail;                    // bytes of a block record (4 Dc + 384), full code granules (Dc / 128), Dc % 128 == 64
    uint32_t ex16;                              // 16-byte units of one slot's ex code (0: 1-bit index)
    SlotArrays src, dst;
};
hipError_t launch_remove_gather(const RemoveGatherParams& P, int device, hipStream_t s);

// ---- fetch_embedding (k_fetch.hip) -------------------------------------------------------------------------------------------
// id map: the (id, slot) pairs of every real slot in (cluster, position) order, stably sorted by id.  vstart [n_lists + 1] =
// exclusive prefix of list_n (host); ids_out / slots_out hold n_vectors entries.  tmp == null returns the scratch size in *tmp_bytes.
hipError_t launch_fetch_gather(const uint64_t* vstart, const uint32_t* list_gb0, uint32_t n_lists, const uint64_t* slot_ids,
                               uint64_t n_vectors, uint64_t* ids_out, uint32_t* slots_out, hipStream_t s);
hipError_t sort_pairs_u64_u32(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in,
                              uint32_t* vals_out, size_t n, hipStream_t s);
struct FetchParams {
    const uint64_t* map_ids;    // [n_map] ascending
    const uint32_t* map_slots;  // [n_map]
    uint64_t n_map;
    const uint32_t* list_gb0;   // [n_lists]
    const float* centroids;     // [n_lists][D] rotated
    const uint8_t* blocks;      // device block records (stride Dc * 4 + 384)
    const uint8_t* ex;          // lane-major ex codes, exd bytes per slot (ex_bits > 0)
    const float *delta, *vl;    // slot order
    const uint8_t* rot_blob;    // FHT-Kac: 4 x D / 8 flip bytes; Matrix: [D][D] f32 row-major
    uint64_t exd;
    uint32_t n_lists, dim, D, Dc, ex_bits, cpu, rotator, trunc;
    float rfac, rlen;           // 1 / fac and 1 / (FHT length), f32 divisions on the host
};
// n ids -> out [n][dim] f32, found [n] u8 (a missing id: zero row, 0).  Matrix rotator: `rows` is [n][D] f32 scratch.
hipError_t launch_fetch(const FetchParams& P, const uint64_t* ids, uint64_t n, float* out, uint8_t* found, float* rows,
                        hipStream_t s);
// The Matrix rotator's inverse alone (k_fetch_matrix): out[v][col] = found[v] ? sum over r of R[r][col] * rows[v][r] : 0
hipError_t launch_fetch_matrix(const float* R, const float* rows, const uint8_t* found, uint64_t n, uint32_t D, uint32_t dim, float* out,
                               hipStream_t s);

// ---- rbq_bf_remove_ids / rbq_bf_fetch_embeddings (k_bf_mutate.hip; include/rbq_bf_mutate.h) -----------------
// keep[i] = 0 for every i = ids[j] < n; the caller fills keep [n] with ones first (ids are positions: no sort)
hipError_t launch_bf_mark(const uint64_t* ids, uint64_t n_ids, uint64_t n, uint8_t* keep, hipStream_t s);
// rank[i] = kept rows (keep[j] != 0) before row i, i < n; tmp == null returns the scratch size in *tmp_bytes.  The caller scans
// one entry more than the index has rows (keep's last entry 0): rank's last value is the number of survivors.
hipError_t bf_scan_kept(void* tmp, size_t* tmp_bytes, const uint8_t* keep, uint32_t* rank, uint64_t n, hipStream_t s);
// map[rank[i]] = i for every kept row i < n
hipError_t launch_bf_row_map(const uint8_t* keep, const uint32_t* rank, uint64_t n, uint32_t* map, hipStream_t s);
// The flat arrays of a brute-force index gathered into those of a shrunk one: new row r takes old row map[r] — its sign code
// (bin_len bytes), its ex code (ex_len bytes; 0: none held) and its eight factors.
struct BfGatherParams {
    const uint32_t* map; // [n_new], ascending, every entry < n_old
    uint64_t n_new, n_old;
    uint32_t bin_len, ex_len;
    const uint8_t *bin_s, *ex_s;
    uint8_t *bin_d, *ex_d;
    const float* f_s[8];
    float* f_d[8];
};
hipError_t launch_bf_gather(const BfGatherParams& P, int device, hipStream_t s);
// fetch_embedding against the zero centroid from the flat layout: n ids -> out [n][dim] f32, found [n] u8 (an id >= n_vectors:
// zero row, 0).  Matrix rotator: `rows` is [n][D] f32 scratch, and launch_fetch_matrix follows.
struct BfFetchParams {
    const uint8_t *bin, *ex;  // [n_vectors][D / 8] MSB-first sign bits; [n_vectors][D * ex_bits / 8] cpp-compat ex codes
    const float *delta, *vl;  // [n_vectors]
    const uint8_t* rot_blob;  // FHT-Kac: 4 x D / 8 flip bytes; Matrix: [D][D] f32 row-major
    uint64_t n_vectors;
    uint32_t dim, D, ex_bits, rotator, trunc;
    float rfac, rlen;         // 1 / fac and 1 / (FHT length), f32 divisions on the host
};
hipError_t launch_bf_fetch(const BfFetchParams& P, const uint64_t* ids, uint64_t n, float* out, uint8_t* found, float* rows,
                           hipStream_t s);

} // namespace rbq
