// bf_range.hpp — kernels of the brute-force range search (rbq_bf_range_batch, include/ext/rbq_bf_range.h):
// every vector whose distance is finite and below a radius, in id order.  They run behind k_bf_dist (bf.hpp), which fills the
// [nq][nv] f32 workspace of a (query sub-batch, vector chunk) with the crate's distances, NaN for a filtered-out vector.
//
// A query's row of the workspace is cut into spans of kBfRangeSpan vectors; one workgroup of 256 threads owns a (span, query):
//
//   k_bf_range_count  reads the span (kBfRangeRounds loads per lane, all in flight before the first compare), reduces the ballot
//                     popcounts of its four waves and writes one u32 to span_counts[q][span].
//   k_bf_range_place  base = the query's running total of the earlier chunks + span_counts[q][0 .. span), summed by the whole
//                     workgroup.  It reads the span again; the hit of round u, wave w, lane l goes to
//                       base + hits of rounds < u + hits of waves < w in round u + popcount(ballot & lanes below l)
//                     which is its rank among the query's matches in id order.  A position below `capacity` gets the id and the
//                     score, a later one is only counted.  The same sum taken over every span gives the chunk's total, so every
//                     workgroup knows it: the one of the last span hands the new running total to the next chunk, and on the
//                     last chunk the workgroups share out the unused slots [min(total, capacity), capacity) of the row.
//
// Every position is a sum of counts that an earlier launch or this workgroup itself has written: no atomic, no workgroup that
// waits on another, and the same rows from run to run.  The running totals alternate between two arrays from chunk to chunk
// (run_in is read by every workgroup of a query while the last one writes run_out).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "bf_range_span.hpp" // kBfRangeThreads / Rounds / Waves, bf_range_load, bf_range_hit: shared with k_bf_range_exact
#include "range_common.hpp"  // rg_pad_row

namespace rbq {

// grid: (n_spans, nq); block kBfRangeThreads
__global__ __launch_bounds__(kBfRangeThreads) void k_bf_range_count(BfRangeParams P) {
    __shared__ uint32_t s_w[kBfRangeWaves];
    const uint32_t tid = threadIdx.x, span = blockIdx.x, q = blockIdx.y;
    float dv[kBfRangeRounds];
    bf_range_load(P, q, span, tid, dv);
    uint32_t c = 0; // wave-uniform
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) c += (uint32_t)__popcll(__ballot(bf_range_hit(dv[u], P.radius)));
    if ((tid & 63u) == 0) s_w[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBfRangeWaves; ++w) t += s_w[w];
        P.span_counts[(size_t)q * P.n_spans + span] = t;
    }
}

// grid: (n_spans, nq), or (1, nq) when P.capacity == 0 (count only: the workgroup stands for the last span and reads no
// distance); block kBfRangeThreads
__global__ __launch_bounds__(kBfRangeThreads) void k_bf_range_place(BfRangeParams P) {
    __shared__ uint32_t s_sum[2][kBfRangeWaves];
    __shared__ uint32_t s_cnt[kBfRangeRounds][kBfRangeWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.y;
    const uint32_t cap = P.capacity;
    const uint32_t span = cap ? blockIdx.x : P.n_spans - 1u;
    float dv[kBfRangeRounds];
    if (cap) bf_range_load(P, q, span, tid, dv); // in flight under the reduction below

    // hits of the spans before this one, and of all spans of the chunk
    const uint32_t* sc = P.span_counts + (size_t)q * P.n_spans;
    uint32_t before = 0, all = 0;
    for (uint32_t j = tid; j < P.n_spans; j += kBfRangeThreads) {
        const uint32_t c = sc[j];
        all += c;
        before += j < span ? c : 0u;
    }
    before = wave_sum_u32(before);
    all = wave_sum_u32(all);
    if (lane == 0) { s_sum[0][wave] = before; s_sum[1][wave] = all; }

    uint64_t bal[kBfRangeRounds]; // wave-uniform
    if (cap) {
#pragma unroll
        for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
            bal[u] = __ballot(bf_range_hit(dv[u], P.radius));
            if (lane == 0) s_cnt[u][wave] = (uint32_t)__popcll(bal[u]);
        }
    }
    __syncthreads();
    const uint32_t carried = P.first ? 0u : P.run_in[q];
    uint32_t base = carried, total = carried;
#pragma unroll
    for (uint32_t w = 0; w < kBfRangeWaves; ++w) { base += s_sum[0][w]; total += s_sum[1][w]; }
    if (tid == 0 && span + 1u == P.n_spans) {
        if (P.last) P.out_counts[q] = total;
        else P.run_out[q] = total;
    }
    if (!cap) return;

    uint64_t* oid = P.out_ids + (size_t)q * cap;
    float* osc = P.out_scores + (size_t)q * cap;
    if (base < cap) { // (else every hit of this span is past the row's end: counted above, nothing to write)
        const uint64_t id0 = P.v0 + (uint64_t)span * kBfRangeSpan + tid;
        uint32_t pos = base; // first position of the round
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
            const uint32_t p = pos + lower + below;
            if (bf_range_hit(dv[u], P.radius) && p < cap) {
                oid[p] = id0 + kBfRangeThreads * u;
                osc[p] = P.metric == 0 ? dv[u] : -dv[u];
            }
            pos += round;
        }
    }
    if (P.last) { // the unused slots of the row, an equal piece per workgroup
        const uint32_t lo = total < cap ? total : cap;
        const uint32_t piece = (cap - lo + P.n_spans - 1u) / P.n_spans;
        const uint64_t a = (uint64_t)lo + (uint64_t)span * piece;
        const uint64_t b = a + piece < cap ? a + piece : cap;
        rg_pad_row(oid, osc, a, b, tid, kBfRangeThreads);
    }
}

} // namespace rbq
