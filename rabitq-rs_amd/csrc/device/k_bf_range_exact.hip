// k_bf_range_exact.hip — translation unit of the exact brute-force range search's kernel (bf_range_exact.hpp) and its launcher: six
// instantiations, metric x element type of the raw rows.  gfx950 only.
#include <hip/hip_runtime.h>

#include "launch_util.hpp" // raw_rows_by_element, dispatch_raw_dtype

#pragma clang fp contract(off)

#include "rerank_score.hpp" // (after the pragma: the scorer's sums are unfused)
#include "bf_range_exact.hpp"

namespace rbq {

namespace {
template <int RAW>
hipError_t launch_bfx(const BfRangeExactParams& P, hipStream_t s) {
    const dim3 grid(P.n_spans, P.nq), block(kBfRangeThreads);
    if (P.metric == 1) hipLaunchKernelGGL((k_bf_range_exact<true, RAW>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((k_bf_range_exact<false, RAW>), grid, block, 0, s, P);
    return hipGetLastError();
}
} // namespace

hipError_t launch_bf_range_exact(const BfRangeExactParams& P0, hipStream_t s) {
    BfRangeExactParams P = P0;
    if (P.nq == 0u || P.nv == 0u || P.dim == 0u || P.dim > kBfRangeExactMaxDim || !P.raw || !P.dist || !P.queries || !P.span_counts ||
        (uint64_t)P.n_spans * kBfRangeSpan < P.nv || (uint64_t)(P.n_spans - 1u) * kBfRangeSpan >= P.nv)
        return hipErrorInvalidValue;
    P.raw_by_element = raw_rows_by_element(P.raw, P.raw_dtype, P.dim);
    return dispatch_raw_dtype(P.raw_dtype, [&](auto raw) { return launch_bfx<decltype(raw)::value>(P, s); });
}

} // namespace rbq
