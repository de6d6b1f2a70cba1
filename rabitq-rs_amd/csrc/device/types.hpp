// types.hpp — plain data shared by the host side (api_*.hip) and the kernel translation units
// (k_query.hip, k_scan.hip, k_build.hip): kernel parameter blocks, device record layouts, launch geometry.
// No device code in here, so the host TU can include it without instantiating a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hl_layout.hpp"
#include "../host/rbq_scan_limits.hpp"

namespace rbq {

constexpr int kThreads = 256;
// element type of the attached raw rows and of a call's query rows: the values of RBQ_RAW_* (rbq.h); a 16-bit element widens to
// an f32 exactly
constexpr int kRawF32 = 0, kRawF16 = 1, kRawBf16 = 2;
constexpr size_t raw_elem_bytes(int raw_dtype) { return raw_dtype == kRawF32 ? 4 : 2; }

// numeric variants (RBQ_NUMERIC_* of rbq.h; kernels.hpp says what each reproduces)
enum : int { kVarAvx512 = 0, kVarAvx2 = 1, kVarPortable = 2 };

struct QueryConsts {
    float delta, sum_vl, k1x, kbx, scale, qnorm;
    float qnorm2;     // |q|^2 of the rotated query (approximate ranking, rank_mfma.hpp)
    float exlo, exhi; // the ex-code dot product sum_i code_i * q_i of ANY code (code_i in [0, 2^ex - 1]) lies in [exlo, exhi],
                      // rounding of the kernel's own summation included (lazy probe selection, select_mfma.hpp)
    float q1norm;     // sum_i |q_i| of the rotated query (rounding slack of that selection)
    float amin, amax; // sum over codebooks of the smallest / largest u8 entry: accu of ANY code lies in [amin, amax]
};
struct ProbeInfo {
    float g_add, g_err, dotqc;
    uint32_t cid;
};
struct WorkItem {
    uint32_t gblock;      // global 32-vector block index
    uint32_t rank_nvalid; // (probe rank << 6) | number of real vectors in the block (1..32)
};
// Per-block factor ranges over the block's REAL vectors, computed once at index creation.  Every float op of
// the epilogue is monotone in each operand, so evaluating it on these extremes brackets every lane's lower
// bound: lbmin <= lb_v <= lbmax.  `usable` is 0 when any factor is non-finite (the block is then never skipped).
struct BlockSummary {
    float fadd_min, fadd_max, fres_min, fres_max, ferr_min, ferr_max;
    uint32_t usable, pad;
};
// Per-block maxima over the block's REAL vectors of the quantities that bound, by Cauchy-Schwarz around the list's
// centroid, the refined distance and the 1-bit estimate of every vector for ANY query (k_list_summaries, encode.hpp):
//   refined distance <= S + g_add + B * g_err,   1-bit estimate <= S1 + g_add + B1 * g_err   (+ rounding slack, block_ub()).
// fadd_ex_abs / fres_ex_abs: largest |f_add_ex| / |f_rescale_ex| (magnitudes for that slack).  usable = 0: a factor of the
// block is not finite (the block then proves nothing).
struct BlockSummaryEx {
    float S, B, S1, B1, fadd_ex_abs, fres_ex_abs;
    uint32_t usable, pad;
};
// TEST ONLY: multipliers of the rounding-slack terms of block_ub() (kernels.hpp), all 1 in the product.  A test scales one term at a
// time (debug options slack_term / slack_milli) and asks the lazy_audit check whether the selection still drops only lists the
// reference skips: a term scaled far below zero must make the audit fire — the audit sees every term.
struct SlackMul {
    float ge = 1.0f;   // 0: |q - c| <= g_err (1 + 1e-4)
    float eip = 1.0f;  // 1: E_ip, the u8 quantisation of the LUT + the sequential f32 sums
    float est = 1.0f;  // 2: 1e-5 of the magnitudes of the 1-bit estimate's operations
    float lb = 1.0f;   // 3: 1e-5 |f_error| g_err of the lower bound's last operation
    float et = 1.0f;   // 4: 1e-3 (2^ex - 1) |q|_1, the f32 summation of the ex-code dot
    float dist = 1.0f; // 5: 1e-5 of the magnitudes of the refined distance's operations
};
// One entry of a query's block stream (probe order, block order within a list).  `lbmin` is the block-level
// lower bound of this (query, block) pair — everything in it but the running threshold is known when the
// stream is written, so the scan's fill step is one 16-byte load and one compare per block.
struct StreamItem {
    uint32_t gblock, rank_nvalid;
    float lbmin; // -inf: never skip
    uint32_t pad;
};

// round-to-nearest-even f32 -> bf16 bits (inf stays inf; NaN stays NaN)
__host__ __device__ inline uint16_t bf16_rne(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u); // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf16_to_f32(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// x = hi + lo + r: the subtraction is exact (hi is x rounded to 8 significant bits)
__host__ __device__ inline void bf16_split(float x, uint16_t& hi, uint16_t& lo) {
    hi = bf16_rne(x);
    lo = bf16_rne(x - bf16_to_f32(hi));
}
// (the interleaved image of the two planes that the ranking GEMM reads: hl_layout.hpp, hl_offset)

// One-product f16 operands of the ranking GEMM (k_rank_f16_db): round-to-nearest-even f32 -> f16 bits, and every result below the
// smallest normal half (2^-14) stored as a signed zero, so that the MFMA never meets a subnormal whatever the denormal mode.
// Values that round to 2^16 or more become inf, NaN stays NaN.  (|x| in [2^-14 - 2^-25, 2^-14) rounds UP to the smallest normal at
// the subnormal spacing 2^-24, ties to even: what IEEE conversion followed by the flush gives.)
__host__ __device__ inline uint16_t f16_rne_flush(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                         // NaN
    if (u < 0x38800000u) return (uint16_t)(sign | (u >= 0x387fe000u ? 0x0400u : 0u)); // below 2^-14
    u += 0xfffu + ((u >> 13) & 1u);
    if (u >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                        // 2^16 and beyond
    return (uint16_t)(sign | ((u - 0x38000000u) >> 13));
}
__host__ __device__ inline float f16_to_f32(uint16_t h) { // (images only: no subnormal halves)
    const uint32_t m = h & 0x7fffu;
    uint32_t u = ((uint32_t)(h & 0x8000u) << 16) | (m >= 0x7c00u ? 0x7f800000u | ((m & 0x3ffu) << 13) : (m ? (m << 13) + 0x38000000u : 0u));
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// image element and its residual x - f16(x): exact in f32 (a stored normal half is within a factor 2 of x — Sterbenz; a flushed one
// leaves x itself); not finite when the image is not
__host__ __device__ inline uint16_t f16_image(float x, float& resid) {
    const uint16_t h = f16_rne_flush(x);
    resid = x - f16_to_f32(h);
    return h;
}

// ---- k_scan ---------------------------------------------------------------------------------------------------
struct ScanParams {
    const uint8_t* blocks;   // [n_blocks][4Dc + 384]: lane-major sign codes | f_add[32] | f_rescale[32] | f_error[32]
    const uint64_t* ids;     // [n_blocks*32]
    const uint8_t* ex_codes; // [n_blocks*32][ex_bytes_dev]: lane-major ex codes, see ex_w4()
    const float* f_add_ex;   // [n_blocks*32]
    const float* f_rescale_ex;
    const uint8_t* lut;      // [nq][4Dc] (pair-swapped codebook order); Dc = D rounded up to x64
    const float* rot;        // [nq][D]
    const QueryConsts* consts;
    const ProbeInfo* probe;  // [nq][nprobe]
    const StreamItem* wl;    // [nq][wl_stride]
    const uint32_t* nstream; // [nq]
    const uint32_t* filter;  // dense bitset or null
    uint64_t filter_nbits;
    uint64_t wl_stride;
    uint64_t* out_ids;
    float* out_scores;
    uint32_t* out_counts;
    unsigned long long* diag; // [nq][3] or null
    uint32_t D, Dc, nprobe, top_k, metric, ex_bits;
    uint32_t no_block_bound; // diagnostic: stream every probed block (measures the pure streaming rate)
    uint32_t exact_heap;     // diagnostic: emulate the reference's BinaryHeap from the start (no sorted fast path)
    unsigned int* heap_restarts; // counter of queries re-run with the exact heap after a distance tie (or null)
    uint32_t mstg;           // MSTG posting-list semantics (src/mstg/index.rs:216-330): distance = binary estimate,
                             // non-finite dropped, L2 clamped to >= 0, no error-bound term
    unsigned long long* prof; // null, or the traffic counters [kProfStripes][kProfSlots] of kProf* below (added once per workgroup, at exit)
    uint32_t* heap_ws;            // null, or [nq][2 * (top_k + 1)] words: the exact heap in global memory (top_k beyond the LDS)
    const uint32_t* dead_skipped; // [nq] vectors of probed lists that the probe selection proved skipped as a whole (they
                                  // never enter the stream; diagnostics add them to skipped_by_lower_bound), or null
    uint32_t wave_kernel;         // 1: k_scanw (one wave per query, scanw.hpp) where it serves the call; 0: k_scan (one workgroup per query)
    // k_scan: log of the candidates the fast pass refined (lower bound, distance, slot — in stream order, tie_log_cap entries per
    // query), or null.  A query whose result depends on the layout of the reference's BinaryHeap (equal distances) then replays the
    // LOG through the exact heap instead of scanning its lists again; a log that overflowed falls back to the re-scan.
    uint32_t* tie_log;
    uint32_t tie_log_cap;
    unsigned int* tie_stats;      // [4] counters: replays, entries replayed, real heap operations, overflowed logs (or null)
    uint32_t numeric_variant;     // host-side dispatch only: kVarAvx512 / kVarAvx2 / kVarPortable (kernels.hpp) picks the
                                  // instantiation; the kernels never read it
};
// traffic counters kept while a profile is open (rbq_profile_begin/end); [0] is written by the select kernels
enum { kProfVectorsProbed = 0, kProfCodeBlocks = 1, kProfMetaBlocks = 2, kProfStreamEntries = 3, kProfExEvals = 4,
       kProfQueries = 5, kProfSlots = 8 };
// The counters are kept in kProfStripes copies (one 64-byte line each), a query adds to copy (query index mod kProfStripes) and
// the host sums them: six atomics per query on ONE address serialise in the L2 and were 9 % of the pipelined rate (round 3).
constexpr uint32_t kProfStripes = 64;
__host__ __device__ inline uint32_t prof_stripe(uint32_t q) { return (q % kProfStripes) * (uint32_t)kProfSlots; }

// kNScan .. kQueueCap, the top_k / nprobe / LDS limits, the ex-code layout arithmetic and scan_lds_bytes: host/rbq_scan_limits.hpp
// (included above: the host's routing plan reads the same definitions)

// blocks per scanner half-wave and tile of k_scan<DT, ...>: two for the compile-time dimensions up to 256 (DT = 0: runtime dimension)
// (Measured in round 3 and left OFF: -DRBQ_SCAN_NB_MAXDIM=256 gives two blocks per half-wave and tile at D <= 256 — parity green,
// but cfg2 (d = 128) 5.78 M queries/s against 6.25 M with one block, streaming roofline 0.312 against 0.318: the tile needs
// 120 registers (4 waves per SIMD instead of 5) and the per-tile hand-over was not what bounds it.)
#ifndef RBQ_SCAN_NB_MAXDIM
#define RBQ_SCAN_NB_MAXDIM 0
#endif
#ifndef RBQ_SCAN_NB
#define RBQ_SCAN_NB 2
#endif
__host__ __device__ constexpr int scan_nb(uint32_t DT) { return (DT != 0 && DT <= RBQ_SCAN_NB_MAXDIM) ? RBQ_SCAN_NB : 1; }
static_assert(RBQ_SCAN_NB * kTileBlocks - 1 + kWindow <= kQueueCap, "live queue too small");

// ---- k_range (range.hpp): every probed vector within a radius ---------------------------------------------------------------
// The scan's parameters with top_k read as the CAPACITY of a query's output row, and the constant threshold R that stands where the
// reference's running `distk` does (R = r for L2, -r for inner product).  heap_ws, tie_log, dead_skipped, exact_heap, wave_kernel
// and prof are not read.
struct RangeParams : ScanParams {
    float R = 0.0f;
};
constexpr int kRangeThreads = 256;                   // four waves, all scanning
constexpr int kRangeBlocks = kRangeThreads / 32;     // stream entries per tile: one per half-wave
constexpr int kRangeCand = kRangeBlocks * 32;        // candidates per tile
// LDS carve-up of k_range (dynamic only, LUT at byte 0):
//   lut[4Dc] u8 | qrot[ex_qlen] f32 | slot, ip, gadd, d [kRangeCand] (a tile's survivors, stream order) |
//   mask[2][kRangeBlocks] u32 | wave counts [8] u32 | nskip + pad [4] u32
__host__ __device__ inline size_t range_lds_bytes(uint32_t Dc, uint32_t D, uint32_t ex_bits) {
    return (size_t)Dc * 4 + (size_t)ex_qlen(D, ex_bits) * 4 + (size_t)kRangeCand * 16 + 2 * (size_t)kRangeBlocks * 4 + 8 * 4 + 4 * 4;
}
// The exact range scan (options range_exact / range_exact_radius_bits): k_range<..., XR, XIP> scores every match
// of the estimate exactly against its raw row and keeps those whose exact score passes X.  XR = kRangeEstimate: today's kernel, which
// takes RangeParams and reads nothing of what follows.
constexpr int kRangeEstimate = -1;
struct RangeExactParams : RangeParams {
    const void* queries = nullptr; // [nq][dim] elements of query_dtype: the caller's unrotated queries
    const void* raw = nullptr;     // [n_raw][dim] elements of raw_dtype (n_raw >= 1)
    uint64_t n_raw = 0;
    uint32_t dim = 0;
    int query_dtype = kRawF32;
    int raw_dtype = kRawF32;       // host-side dispatch only: picks the instantiation
    uint32_t raw_by_element = 0;   // set by the launch: 16-bit rows that do not all start 4-byte aligned (odd dim, or raw at 2 mod 4)
    float X = 0.0f;                // a candidate matches iff exact distance < X (L2) or exact dot > X (inner product)
};
// LDS carve-up of the exact variant: k_range's region above (a multiple of 16 bytes), then
//   id[kRangeCand] u64 (a tile's matches of the estimate, stream order) | exact score[kRangeCand] f32 | hits per wave [4] u32 |
//   query[dim] f32 (the caller's, widened)
// 8 KiB of LUT + 8 KiB of rotated query + 4 KiB of survivors + 3 KiB + 8 KiB of query at padded_dim 2048, of the CU's 160 KiB.
__host__ __device__ inline size_t range_exact_lds_bytes(uint32_t Dc, uint32_t D, uint32_t ex_bits, uint32_t dim) {
    return range_lds_bytes(Dc, D, ex_bits) + (size_t)kRangeCand * 12 + 4 * 4 + (size_t)dim * 4;
}

// ---- encoder ----------------------------------------------------------------------------------------------------
constexpr uint32_t kNoSrc = 0xffffffffu;
struct EncodeParams {
    const float* rows;          // [nrows][D] rotated vectors of this chunk
    const float* centroids;     // [nlist][D] rotated
    const uint32_t* slot_src;   // block-ordered mode: [nslots] source vector index or kNoSrc (chunk-local view)
    const uint32_t* block_list; // list of every block (block-ordered mode: chunk-local view; scatter mode: global)
    const uint32_t* row_slot;   // scatter mode: [nrows] global slot of row r (null = block-ordered mode, slot = r)
    uint8_t* blocks;            // block records (block-ordered mode: chunk-local view; scatter mode: whole array)
    uint8_t* raw_ex;            // [nrows][D] u8 scratch (ex_bits > 0)
    float* f_add_ex;            // like `blocks`
    float* f_rescale_ex;
    float* delta;               // reconstruction factors delta / vl, slot order like f_add_ex (null: not written)
    float* vl;
    uint64_t* ids;
    uint64_t src_base;          // ids[slot] = src_base + source index (scatter mode: src_base + row)
    uint32_t nslots, D, Dc, ex_bits, metric;
    float t_const;
    const double* t_row;        // optimal rescale (k_encode<*, true>): [nrows] t of every row (k_rescale); else unused
    // flat mode (k_encode<false, *, true>, the brute-force index): `blocks` is bin[nslots][D/8]; slot_src, block_list, centroids
    // and ids are unused; f_add_ex, f_rescale_ex, delta, vl and the four arrays below are the index's per-vector factors
    // (residual_norm alone, in the block-ordered mode: slot order like delta — MSTG handles; null: not written)
    float *f_add = nullptr, *f_rescale = nullptr, *f_error = nullptr, *residual_norm = nullptr;
};
constexpr int kEncThreads = 64;          // 64 vectors = 2 blocks per workgroup

} // namespace rbq
