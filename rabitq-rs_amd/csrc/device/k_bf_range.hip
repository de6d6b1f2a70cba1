// k_bf_range.hip — translation unit of the brute-force range search's kernels (bf_range.hpp) and their launchers.  gfx950 only.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "bf_range.hpp"

namespace rbq {

hipError_t launch_bf_range_count(const BfRangeParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_bf_range_count, dim3(p.n_spans, p.nq), dim3(kBfRangeThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_bf_range_place(const BfRangeParams& p, hipStream_t s) {
    // count only: one workgroup per query sums the span counts
    hipLaunchKernelGGL(k_bf_range_place, dim3(p.capacity ? p.n_spans : 1u, p.nq), dim3(kBfRangeThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace rbq
