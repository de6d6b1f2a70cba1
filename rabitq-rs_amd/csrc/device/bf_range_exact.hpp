// bf_range_exact.hpp — the kernel of the exact brute-force range search (rbq_bf_range_exact_batch, include/ext/rbq_bf_range.h;
// DESIGN.md section 41).  It runs in k_bf_range_count's place of the chain k_bf_dist -> count -> k_bf_range_place (bf_range.hpp),
// with that chain's split: one workgroup of 256 threads owns one (span of kBfRangeSpan vectors, query).
//
//   k_bf_range_exact<IP, RAW>   RAW: the element type of the raw rows (kRawF32 / kRawF16 / kRawBf16).
//     1  the lane's 8 estimates of the span are loaded (bf_range_load); while they travel the query's raw f32 row goes to LDS;
//     2  8 ballots against the candidate radius r, their 8 x 4 wave popcounts meet in LDS behind one barrier;
//     3  a candidate's position in the span goes, as a u16, to slot
//          hits of rounds < u + hits of waves < w in round u + popcount(ballot & lanes below)
//        of a list of 2048 entries in LDS — k_bf_range_place's rank arithmetic, so the list is in id order.  In the same step every
//        entry that is no candidate is overwritten with the NaN 0x7fc00000 in the workspace;
//     4  ceil(count / 32) passes, the same number on every wave.  In pass p the group g = 8 wave + lane / 8 of eight lanes scores
//        candidate 32 p + g with rp_score_row (rerank_score.hpp: the bits of canon_l2 / canon_dot); a group without a candidate
//        scores row 0 and discards it.  The group's first lane writes d (canon_l2, or -canon_dot) over the candidate's estimate;
//     5  the ballots of (candidate && d finite && d < x) are popcounted per wave, the four sums meet in LDS, one u32 goes to
//        span_counts[q][span].
//   k_bf_range_place, unchanged, then runs with radius = x over the overwritten workspace: placement in id order, the totals
//   carried across chunks, the count-only form and the tail fill are its.
//
// Every raw row is read at most once per query; no atomic decides a position; no workgroup waits on another; every entry of the
// workspace is written only by the workgroup that owns its span.  No matrix instruction: the sums follow the crate's serial
// order, eight chains per row, which an MFMA's internal order of additions cannot reproduce.
// Static LDS: query 8192 + list 4096 + popcounts 128 + wave sums 16 bytes.
//
// The including unit sets #pragma clang fp contract(off) in front of this header (the scorer's d * d and + stay apart).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "bf_range_span.hpp" // kBfRangeThreads / Rounds / Waves, bf_range_load, bf_range_hit: shared with bf_range.hpp
#include "rerank_score.hpp"  // rp_score_row

namespace rbq {

static_assert(kBfRangeSpan <= 65536, "a position in a span fits a u16");

// grid: (n_spans, nq); block kBfRangeThreads.  Every candidate's id is below v0 + nv, so its raw row exists.
template <bool IP, int RAW>
__global__ __launch_bounds__(kBfRangeThreads) void k_bf_range_exact(BfRangeExactParams P) {
    __shared__ __align__(16) float s_q[kBfRangeExactMaxDim];
    __shared__ uint16_t s_pos[kBfRangeSpan];
    __shared__ uint32_t s_cnt[kBfRangeRounds][kBfRangeWaves];
    __shared__ uint32_t s_w[kBfRangeWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, span = blockIdx.x, q = blockIdx.y, dim = P.dim;
    float* row = P.dist + (size_t)q * P.nv + (size_t)span * kBfRangeSpan; // the span's entries of the workspace
    const uint64_t left = P.nv - (uint64_t)span * kBfRangeSpan;           // ... of which this many exist (>= 1)

    // ---- 1
    float dv[kBfRangeRounds];
    bf_range_load(P, q, span, tid, dv);
    const float* qrow = P.queries + (size_t)q * dim;
    for (uint32_t i = tid; i < dim; i += kBfRangeThreads) s_q[i] = qrow[i];

    // ---- 2
    uint64_t bal[kBfRangeRounds]; // wave-uniform
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        bal[u] = __ballot(bf_range_hit(dv[u], P.candidate_radius));
        if (lane == 0) s_cnt[u][wave] = (uint32_t)__popcll(bal[u]);
    }
    __syncthreads();

    // ---- 3
    uint32_t count = 0; // candidates of the rounds so far; after the loop: of the span (the same on every thread)
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        uint32_t lower = 0, round = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBfRangeWaves; ++w) {
            const uint32_t c = s_cnt[u][w];
            lower += w < wave ? c : 0u;
            round += c;
        }
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[u], 0u));
        const uint32_t at = kBfRangeThreads * u + tid; // position in the span
        if (bf_range_hit(dv[u], P.candidate_radius)) s_pos[count + lower + below] = (uint16_t)at;
        else if (at < left) row[at] = __int_as_float(0x7fc00000);
        count += round;
    }
    __syncthreads();

    // ---- 4 and 5
    const uint32_t j = lane & 7u, base = lane & ~7u, grp = wave * 8u + (lane >> 3);
    const uint64_t id0 = P.v0 + (uint64_t)span * kBfRangeSpan;
    const bool by_element = P.raw_by_element != 0u;
    const uint32_t passes = (count + 31u) / 32u; // (the same on every wave: the scorer's lanes exchange data inside their wave)
    uint32_t hits = 0;                            // wave-uniform
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t c = 32u * p + grp;
        const bool act = c < count;
        const uint32_t at = act ? (uint32_t)s_pos[c] : 0u;
        const float sum = rp_score_row<IP, RAW>(P.raw, id0 + at, act, s_q, dim, j, base, by_element);
        const float d = IP ? -sum : sum;
        const bool first = act && j == 0u;
        if (first) row[at] = d;
        hits += (uint32_t)__popcll(__ballot(first && bf_range_hit(d, P.x)));
    }
    if (lane == 0) s_w[wave] = hits;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBfRangeWaves; ++w) t += s_w[w];
        P.span_counts[(size_t)q * P.n_spans + span] = t;
    }
}

} // namespace rbq
