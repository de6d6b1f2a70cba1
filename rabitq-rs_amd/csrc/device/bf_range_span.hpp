// bf_range_span.hpp — what the kernels of the brute-force range searches share about a span (bf_range.hpp: k_bf_range_count,
// k_bf_range_place; bf_range_exact.hpp: k_bf_range_exact): how a workgroup of kBfRangeThreads threads covers its span of
// kBfRangeSpan vectors of a query's row of the distance workspace, and the match rule.  One copy, so that the count a kernel
// writes to span_counts and the positions k_bf_range_place derives from it cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"

namespace rbq {

constexpr uint32_t kBfRangeThreads = 256;
constexpr uint32_t kBfRangeRounds = kBfRangeSpan / kBfRangeThreads; // 256-vector rounds of a span: the loads a lane has in flight
constexpr uint32_t kBfRangeWaves = kBfRangeThreads / 64;
static_assert(kBfRangeSpan % kBfRangeThreads == 0, "a span is a whole number of 256-vector rounds");

// the lane's kBfRangeRounds distances of its span (NaN past the chunk's end), all loads issued before any is used
// (Params: BfRangeParams or BfRangeExactParams — its dist [nq][nv] and nv)
template <class Params>
__device__ __forceinline__ void bf_range_load(const Params& P, uint32_t q, uint32_t span, uint32_t tid, float (&dv)[kBfRangeRounds]) {
    const float* row = P.dist + (size_t)q * P.nv;
    const uint64_t s0 = (uint64_t)span * kBfRangeSpan;
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        const uint64_t i = s0 + kBfRangeThreads * u + tid;
        dv[u] = i < P.nv ? row[i] : __int_as_float(0x7fc00000);
    }
}

// the match rule, for both metrics: finite and below the radius (never true against a NaN distance)
__device__ __forceinline__ bool bf_range_hit(float d, float r) { return finite_f(d) && d < r; }

} // namespace rbq
