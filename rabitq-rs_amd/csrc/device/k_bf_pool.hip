// k_bf_pool.hip — translation unit of the ranked rerank pool's kernels (bf_pool.hpp) and their launcher.  gfx950 only.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "bf_pool.hpp"

namespace rbq {

hipError_t launch_bf_pool_rank(const BfPoolParams& P, hipStream_t s) {
    // what the kernels assume: the pool's bound, spans that cover the chunk exactly, carried blocks that cover the pool exactly,
    // and every array they touch on this chunk
    const uint32_t carry_blocks = (P.pool + kBfRangeSpan - 1u) / kBfRangeSpan;
    if (P.nq == 0u || P.nv == 0u || P.pool == 0u || P.pool > kBfRerankPoolMax || !P.dist || !P.hist || !P.state || !P.span_counts ||
        (uint64_t)P.n_spans * kBfRangeSpan < P.nv || (uint64_t)(P.n_spans - 1u) * kBfRangeSpan >= P.nv ||
        P.v0 + P.nv > (1ull << 32) || P.n_carry != (P.first ? 0u : carry_blocks) ||
        (!P.first && (!P.carry_in || !P.carry_n_in)) ||
        (P.last ? !P.out_ids || !P.out_counts : !P.carry_out || !P.carry_n_out || P.carry_out == P.carry_in || P.carry_n_out == P.carry_n_in))
        return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(P.hist, 0, (size_t)kBfPoolPasses * P.nq * kBfPoolBins * 4u, s);
    if (e != hipSuccess) return e;
    const dim3 grid(P.n_carry + P.n_spans, P.nq), block(kBfRangeThreads);
    for (uint32_t pass = 0; pass < kBfPoolPasses; ++pass) hipLaunchKernelGGL(k_bf_pool_hist, grid, block, 0, s, P, pass);
    hipLaunchKernelGGL(k_bf_pool_count, grid, block, 0, s, P);
    hipLaunchKernelGGL(k_bf_pool_place, grid, block, 0, s, P);
    return hipGetLastError();
}

} // namespace rbq
