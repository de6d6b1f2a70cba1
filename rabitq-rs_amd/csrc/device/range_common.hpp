// range_common.hpp — the one copy of the steps the range-search kernels share (gfx950, wave64): k_range
// (range.hpp), k_mstg_range / k_mstg_range_distinct (k_mstg_range.hip), k_mstg_range_exact (k_mstg_range_exact.hip) and
// k_bf_range_place (bf_range.hpp).  These are the rules of the range contract, so that the index types cannot drift apart:
//   rg_estimate        the epilogue's operation sequence up to the estimate;
//   rg_pad_row         UINT64_MAX / NaN in the slots of a row behind its entries;
//   wg_scan_excl       the workgroup's exclusive prefix sum;
//   rg_distinct_heads  the distinct-id reduction: one flag, in scan order, per id;
//   rg_walk_flags      the flagged ranks of a thread's word, each at its prefix.
#pragma once
#include "kernels.hpp"
#include "launch.hpp"    // kMstgRangeDistinctMax
#include "mstg_pool.hpp"  // mr_sort, kMrDropped

namespace rbq {

static_assert(kMstgRangeDistinctMax == 16 * kThreads, "rg_distinct_heads / rg_walk_flags: sixteen ranks per thread of one flag word");

// The binary estimate as a function of the accumulator: the epilogue's exact operation sequence (compute_batch_distances_u16; the
// first operation fused or not per numeric variant), one statement per rounding.  *ip: the inner product the ex stage goes on from.
__device__ __forceinline__ float rg_estimate(const QueryConsts& qc, float f_add, float f_rescale, float g_add, float accu_f, bool unfused, float& ip) {
    ip = epi_ip(qc.delta, accu_f, qc.sum_vl, unfused);
    const float tt = ip + qc.k1x;
    const float rs = f_rescale * tt;
    float est = f_add + g_add;
    est = est + rs;
    return est;
}

// The tail of a row: slots [from, to) are unused.  from = min(total, capacity) for a whole row.
template <class I>
__device__ __forceinline__ void rg_pad_row(uint64_t* out_ids, float* out_scores, I from, I to, uint32_t tid, uint32_t nthreads) {
    for (I i = from + tid; i < to; i += nthreads) {
        out_ids[i] = ~0ull;
        out_scores[i] = __int_as_float(0x7fc00000);
    }
}

// exclusive prefix sum of one value per thread over the workgroup (kThreads = four waves); *total: the sum, on every thread.
// s_w [kThreads / 64] in LDS; a second scan over the same s_w needs a barrier between the two.
__device__ __forceinline__ uint32_t wg_scan_excl(uint32_t v, uint32_t* s_w, uint32_t tid, uint32_t* total) {
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63u) s_w[wave] = x;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)(kThreads / 64); ++j) {
        const uint32_t c = s_w[j];
        base += j < wave ? c : 0u;
        sum += c;
    }
    *total = sum;
    return base + x - v;
}

// The distinct-id reduction over the `total` (1 .. kMstgRangeDistinctMax) matches of a scan's row (rids, rest: ids and estimates
// in scan order), by a workgroup of kThreads:
//   A  (id | estimate key << 32 + scan rank) of every match into k1, k2 [kMstgRangeDistinctMax] in LDS, padded to a power of two.
//      The key orders by value: -0.0 and +0.0 share one, so rank decides between them;
//   B  mr_sort by (id, estimate by value, rank): the head of an id run is the match the contract keeps — the smallest estimate,
//      on equal values the earlier in scan order;
//   C  every head sets bit (rank & 15) of word rank >> 4 of s_keep [kThreads] (LDS atomic OR): the flags are back in scan order
//      without a second sort.
// Ends in a barrier: the flags are complete and k1, k2 are free.
__device__ __forceinline__ void rg_distinct_heads(unsigned long long* k1, unsigned long long* k2, uint32_t* s_keep, const uint64_t* rids,
                                                  const float* rest, uint32_t total, uint32_t tid) {
    uint32_t np2 = 1;
    while (np2 < total) np2 <<= 1;
    for (uint32_t i = tid; i < np2; i += kThreads) {
        unsigned long long id = kMrDropped, key = kMrDropped;
        if (i < total) {
            const float e = rest[i];
            const float v = e == 0.0f ? 0.0f : e;
            id = rids[i];
            key = ((unsigned long long)((uint32_t)total_key(v) ^ 0x80000000u) << 32) | i;
        }
        k1[i] = id; k2[i] = key;
    }
    s_keep[tid] = 0u;
    mr_sort<true>(k1, k2, np2, tid);
    for (uint32_t i = tid; i < np2; i += kThreads) {
        const unsigned long long key = k2[i];
        if (key != kMrDropped && (i == 0u || k1[i] != k1[i - 1u])) {
            const uint32_t rank = (uint32_t)key;
            atomicOr(&s_keep[rank >> 4], 1u << (rank & 15u));
        }
    }
    __syncthreads();
}

// Thread t owns bits 0 .. 15 of flags[t], places 16 t .. 16 t + 15: popcount, workgroup prefix sum (shuffles inside a wave, four
// partial sums through s_w), then f(at, place) for every flagged place in ascending order, at = its prefix, while at < limit.
// Returns the number of flags of the workgroup, on every thread.
template <class F>
__device__ __forceinline__ uint32_t rg_walk_flags(const uint32_t* flags, uint32_t* s_w, uint32_t tid, uint32_t limit, F f) {
    uint32_t m = flags[tid], n;
    uint32_t at = wg_scan_excl((uint32_t)__popc(m), s_w, tid, &n);
    while (m && at < limit) {
        f(at, tid * 16u + (uint32_t)__ffs(m) - 1u);
        m &= m - 1u;
        ++at;
    }
    return n;
}

} // namespace rbq
