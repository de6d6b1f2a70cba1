// k_mstg_range_exact.hip — the exact MSTG range search (options mstg_range_exact / mstg_range_exact_bits on rbq_mstg_range_batch*;
// include/ext/rbq_mstg_range.h): the estimate's matches at the candidate radius r are only candidates; they are
// reduced to one entry per id, every distinct id is scored exactly against its raw row, and an id matches iff that distance is
// finite and < x.  Takes the place of k_mstg_range_distinct behind k_mstg_range (k_mstg_range.hip), whose workspace row of
// RBQ_MSTG_RANGE_DISTINCT_MAX entries it reads.  gfx950 only, wave64.
//
//   k_mstg_range_exact<IP, RAW>   one workgroup (4 waves) per query.  RAW: the element type of the raw rows (kRawF32 / kRawF16 / kRawBf16).
//     A - C  the query widened into LDS; rg_distinct_heads (range_common.hpp, k_mstg_range_distinct's copy): one flag in scan order
//        for the candidate the distinct rule keeps of every id;
//     D  rg_walk_flags: the heads' ranks go into a dense list in scan order (the key arrays are free after C: the list and the
//        distances live there);
//     S  eight lanes per distinct id, 32 ids per round, ceil(n / 32) rounds on every wave: rp_score_row (rerank_score.hpp: the bits
//        of canon_l2 / canon_dot) over the query in LDS; the id is the scan's row at the rank.  A group without an id, or with an id
//        >= n_raw, reads row 0 and discards it.  Lane 0 of a group stores the distance bits at the dense place (canon_l2 or
//        -canon_dot; NaN without a raw row) and sets the place's hit bit iff the distance is finite and < x;
//     E  rg_walk_flags over the hit bits: the hits are written at their prefix while that is below the capacity, the total goes to
//        out_counts, the rest of the row is padded.
//     No atomic decides a position: every place is a function of the scan rank alone, so the same call gives the same rows.
//     A query without a match, or with more than the limit, takes none of A to E: 0 or UINT32_MAX, and an empty row.
// Dynamic LDS: query[dim rounded up to 2] f32 | k1[4096] u64 | k2[4096] u64 | keep[256] u32 | hit[256] u32 | wave sums [4] u32.
//   k1 after C: the dense list, u32 [4096] (ranks).  k2 after C: the distance bits, u32 [4096], by dense place.
#include <hip/hip_runtime.h>

#include "rbq.h"
#include "ext/rbq_mstg_range.h"
#include "launch_util.hpp"
#include "kernels.hpp"
#include "range_common.hpp" // rg_distinct_heads, rg_walk_flags, rg_pad_row

#pragma clang fp contract(off)

#include "rerank_score.hpp" // (after the pragma: the scorer's sums are unfused)

namespace rbq {

template <bool IP, int RAW>
__global__ __launch_bounds__(kThreads) void k_mstg_range_exact(MstgRangeExactParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    float* sq = reinterpret_cast<float*>(smraw);                                               // [dim]
    unsigned long long* k1 = reinterpret_cast<unsigned long long*>(sq + ((P.dim + 1u) & ~1u)); // A to C: the id
    unsigned long long* k2 = k1 + kMstgRangeDistinctMax;                                       // A to C: estimate key << 32 | scan rank
    uint32_t* s_keep = reinterpret_cast<uint32_t*>(k2 + kMstgRangeDistinctMax); // [kThreads] bit b of word t: rank 16 t + b heads its id
    uint32_t* s_hit = s_keep + kThreads;                                         // [kThreads] bit b of word t: dense place 16 t + b matches
    uint32_t* s_w = s_hit + kThreads;
    uint32_t* dense = reinterpret_cast<uint32_t*>(k1); // D on: [n] the heads' ranks in scan order
    uint32_t* dist = reinterpret_cast<uint32_t*>(k2);  // S on: [n] the reported distance's bits
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, cap = P.cap, dim = P.dim;
    const uint64_t* rids = P.raw_ids + (size_t)q * kMstgRangeDistinctMax;
    const float* rest = P.raw_scores + (size_t)q * kMstgRangeDistinctMax;
    uint64_t* out_ids = P.out_ids + (size_t)q * cap;
    float* out_scores = P.out_scores + (size_t)q * cap;
    const uint32_t total = P.raw_counts[q];
    uint32_t hits = 0;
    if (total != 0u && total <= kMstgRangeDistinctMax) { // (uniform)
        // ---- A to C (every read of the keys is done behind them: their arrays become the dense list and the distances)
        copy_query_widened<kThreads>(sq, P.queries, P.query_dtype, (size_t)q * dim, dim, tid);
        s_hit[tid] = 0u;
        rg_distinct_heads(k1, k2, s_keep, rids, rest, total, tid);
        // ---- D (every head has a place: at < n <= the limit)
        const uint32_t n = rg_walk_flags(s_keep, s_w, tid, kMstgRangeDistinctMax, [&](uint32_t at, uint32_t r) { dense[at] = r; });
        __syncthreads();
        // ---- S: eight lanes per distinct id (a group without one reads row 0 and writes nothing)
        const uint32_t j = lane & 7u, grp = lane >> 3, base = lane & ~7u;
        const uint32_t rounds = (n + 31u) / 32u; // (the same on every wave: the scorer's lanes exchange data inside their wave)
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t p = r * 32u + wave * 8u + grp;
            const bool have = p < n;
            const uint64_t id = have ? rids[dense[p]] : 0ull;
            const bool act = have && id < P.n_raw;
            const float sum = rp_score_row<IP, RAW>(P.raw, id, act, sq, dim, j, base, P.raw_by_element != 0u);
            if (have && j == 0u) {
                const float d = act ? (IP ? -sum : sum) : __int_as_float(0x7fc00000);
                dist[p] = __float_as_uint(d);
                if (finite_f(d) && d < P.X) atomicOr(&s_hit[p >> 4], 1u << (p & 15u)); // (never true against a NaN x)
            }
        }
        __syncthreads();
        // ---- E (p < n: only scored places were flagged)
        hits = rg_walk_flags(s_hit, s_w, tid, cap, [&](uint32_t at, uint32_t p) {
            out_ids[at] = rids[dense[p]];
            out_scores[at] = __uint_as_float(dist[p]);
        });
    }
    rg_pad_row(out_ids, out_scores, hits < cap ? hits : cap, cap, tid, (uint32_t)kThreads);
    if (tid == 0) P.out_counts[q] = total > kMstgRangeDistinctMax ? 0xffffffffu : hits;
}

// Dynamic LDS of one workgroup: the query, 64 KiB of keys, the two flag arrays and the wave sums.  At dim 2048: 8192 + 65536 + 2048
// + 16 = 75792 bytes.
size_t mstg_range_exact_lds_bytes(uint32_t dim) {
    return (size_t)((dim + 1u) & ~1u) * 4 + (size_t)kMstgRangeDistinctMax * 16 + (size_t)kThreads * 8 + 16;
}

namespace {
template <bool IP, int RAW>
hipError_t launch_mrx(const MstgRangeExactParams& P, size_t lds, int device, hipStream_t s) {
    static LdsAttrCache attr;
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_mstg_range_exact<IP, RAW>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mstg_range_exact<IP, RAW>), dim3(P.nq), dim3(kThreads), lds, s, P);
    return hipGetLastError();
}
template <int RAW>
hipError_t launch_mrx(const MstgRangeExactParams& P, size_t lds, int device, hipStream_t s) {
    return P.metric == 1u ? launch_mrx<true, RAW>(P, lds, device, s) : launch_mrx<false, RAW>(P, lds, device, s);
}
} // namespace

hipError_t launch_mstg_range_exact(const MstgRangeExactParams& P0, int device, hipStream_t s) {
    MstgRangeExactParams P = P0;
    if (P.nq == 0u || P.cap == 0u || P.dim == 0u || P.n_raw == 0u || !P.raw) return hipErrorInvalidValue;
    const size_t lds = mstg_range_exact_lds_bytes(P.dim);
    if (lds > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    P.raw_by_element = raw_rows_by_element(P.raw, P.raw_dtype, P.dim);
    return dispatch_raw_dtype(P.raw_dtype, [&](auto raw) { return launch_mrx<decltype(raw)::value>(P, lds, device, s); });
}

} // namespace rbq
