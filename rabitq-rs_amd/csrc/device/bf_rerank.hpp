// bf_rerank.hpp — the two kernels of the exact top-k search on brute-force handles (rbq_bf_search_exact_batch,
// include/ext/rbq_bf_range.h).  They run behind the last k_bf_select of a sub-batch, which has delivered every
// query's pool: the best P = max(pool, top_k) estimates, ascending, as rbq_bf_search_batch returns them at top_k := P.
//
//   k_bf_rerank_score<IP, RAW>   grid (ceil(P / kBfRerankSlice), nq), 256 threads: one workgroup per (slice of 128 pool entries,
//                                query).  RAW: the element type of the raw rows (kRawF32 / kRawF16 / kRawBf16).
//     1  the slice's ids are loaded from k_bf_select's rows, one lane per entry; while they travel the query's f32 row goes to LDS.
//        An id without a raw row (none comes out of the select: the guard keeps every read inside the rows) gets the dropped mark;
//     2  ceil(entries / 32) <= 4 passes, the same number on every wave.  In pass p the group g = 8 wave + lane / 8 of eight lanes
//        scores entry 32 p + g with rp_score_row (rerank_score.hpp: the bits of canon_l2 / canon_dot); a group without an entry
//        scores row 0 and discards it.  The group's first lane writes d (canon_l2, or -canon_dot) to exact[q][entry], the NaN
//        0x7fc00000 for a dropped entry.
//     A slice at or past the query's pool count returns at once.  No atomic, no workgroup waits on another, every raw row is read
//     once per query.  Static LDS: query 8192 + ids 512 bytes.  No matrix instruction: the sums follow the crate's serial order,
//     eight chains per row, which an MFMA's internal order of additions cannot reproduce.
//
//   k_bf_rerank_order            grid nq, 256 threads: one workgroup per query.
//     1  entry r < count becomes k2[r] = order key of d << 32 | id and k1[r] = the bits of d; the key is total_key of d with -0.0
//        taken as +0.0 (k_mstg_rerank's), so it orders by value, and an id is a position below 2^32, so one u64 holds the whole
//        order (d, id).  A non-finite d and the slots up to the power of two at or above the count get kMrDropped, which is
//        above every key of a finite d;
//     2  mr_sort (mstg_pool.hpp) by k2; the survivors are counted by ballots;
//     3  the first min(top_k, survivors) entries are written — the id, and d (L2) or -d (inner product), the scorer's own bits —
//        the other slots UINT64_MAX / NaN 0x7fc00000, and the count.
//     Dynamic LDS: k1[pool_np2] u64 | k2[pool_np2] u64 | 4 u32: 65552 bytes at a pool of 4096.
//
// The including unit sets #pragma clang fp contract(off) in front of this header (the scorer's d * d and + stay apart).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "mstg_pool.hpp"    // mr_sort, kMrDropped
#include "rerank_score.hpp" // rp_score_row

namespace rbq {

constexpr uint32_t kBfRerankThreads = 256;
constexpr uint32_t kBfRerankNoRow = 0xffffffffu; // the dropped mark of an id in LDS (an id is below 2^32 - 1)
static_assert(kBfRerankSlice <= kBfRerankThreads && kBfRerankSlice % 32u == 0u, "one lane loads an entry's id; a pass scores 32 entries");
static_assert(kBfRerankThreads == (uint32_t)kThreads, "mr_sort strides by kThreads");

// grid: (ceil(pool / kBfRerankSlice), nq); block kBfRerankThreads
template <bool IP, int RAW>
__global__ __launch_bounds__(kBfRerankThreads) void k_bf_rerank_score(BfRerankParams P) {
    __shared__ __align__(16) float s_q[kBfRangeExactMaxDim];
    __shared__ uint32_t s_id[kBfRerankSlice];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.y, dim = P.dim;
    const uint32_t cnt = min(P.pool_counts[q], P.pool), e0 = blockIdx.x * kBfRerankSlice;
    if (e0 >= cnt) return; // (the whole workgroup: an empty slice of a pool the filter or the index left short)
    const uint32_t have = min(cnt - e0, kBfRerankSlice);
    float* row = P.exact + (size_t)q * P.pool + e0;

    // ---- 1
    const uint64_t id = tid < have ? P.pool_ids[(size_t)q * P.pool + e0 + tid] : ~0ull;
    const float* qrow = P.queries + (size_t)q * dim;
    for (uint32_t i = tid; i < dim; i += kBfRerankThreads) s_q[i] = qrow[i];
    if (tid < kBfRerankSlice) s_id[tid] = id < P.n_raw ? (uint32_t)id : kBfRerankNoRow;
    __syncthreads();

    // ---- 2
    const uint32_t j = lane & 7u, base = lane & ~7u, grp = wave * 8u + (lane >> 3);
    const bool by_element = P.raw_by_element != 0u;
    const uint32_t passes = (have + 31u) / 32u; // (the same on every wave: the scorer's lanes exchange data inside their wave)
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t c = 32u * p + grp;
        const uint32_t v = c < have ? s_id[c] : kBfRerankNoRow;
        const bool act = v != kBfRerankNoRow;
        const float sum = rp_score_row<IP, RAW>(P.raw, v, act, s_q, dim, j, base, by_element);
        if (c < have && j == 0u) row[c] = act ? (IP ? -sum : sum) : __int_as_float(0x7fc00000);
    }
}

// grid: nq; block kBfRerankThreads; dynamic LDS bf_rerank_order_lds_bytes(P.pool_np2)
__global__ __launch_bounds__(kBfRerankThreads) void k_bf_rerank_order(BfRerankParams P) {
    extern __shared__ __align__(16) unsigned char bfr_lds[];
    unsigned long long* k1 = reinterpret_cast<unsigned long long*>(bfr_lds); // the bits of d, carried along
    unsigned long long* k2 = k1 + P.pool_np2;                                // the order: key of d << 32 | id
    uint32_t* s_fin = reinterpret_cast<uint32_t*>(k2 + P.pool_np2);          // finite survivors
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t cnt = min(P.pool_counts[q], P.pool);
    uint32_t np2 = 1;
    while (np2 < cnt) np2 <<= 1; // <= P.pool_np2
    const uint64_t* pid = P.pool_ids + (size_t)q * P.pool;
    const float* pd = P.exact + (size_t)q * P.pool;
    if (tid == 0) *s_fin = 0u;
    __syncthreads();

    // ---- 1 (every wave runs whole rounds: the ballot counts what its lanes kept)
    for (uint32_t r0 = tid - lane; r0 < np2; r0 += kBfRerankThreads) {
        const uint32_t r = r0 + lane;
        const float d = r < cnt ? pd[r] : __int_as_float(0x7fc00000);
        const bool keep = finite_f(d);
        if (r < np2) {
            const float v = d == 0.0f ? 0.0f : d; // the key orders by value
            const uint32_t key = (uint32_t)total_key(v) ^ 0x80000000u;
            k1[r] = __float_as_uint(d);
            k2[r] = keep ? ((unsigned long long)key << 32) | (uint32_t)pid[r] : kMrDropped;
        }
        const uint32_t kept = (uint32_t)__popcll(__ballot(keep));
        if (lane == 0 && kept) atomicAdd(s_fin, kept);
    }

    // ---- 2
    mr_sort<false>(k1, k2, np2, tid);

    // ---- 3
    const uint32_t n_out = min(*s_fin, P.top_k);
    for (uint32_t i = tid; i < P.top_k; i += kBfRerankThreads) {
        uint64_t id = ~0ull;
        float sc = __int_as_float(0x7fc00000);
        if (i < n_out) {
            const float d = __uint_as_float((uint32_t)k1[i]);
            id = (uint32_t)k2[i];
            sc = P.metric == 1 ? -d : d;
        }
        P.out_ids[(size_t)q * P.top_k + i] = id;
        P.out_scores[(size_t)q * P.top_k + i] = sc;
    }
    if (tid == 0) P.out_counts[q] = n_out;
}

} // namespace rbq
