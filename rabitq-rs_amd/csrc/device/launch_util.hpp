// launch_util.hpp — launch plumbing shared by the range and rerank units (k_range.hip, k_range_exact.hip, k_rerank_pool.hip,
// k_mstg_rerank.hip, k_mstg_range_exact.hip); kept out of launch.hpp so that the other units do not include it.
#pragma once
#include <type_traits>

#include <hip/hip_ext.h>

#include "launch.hpp"

namespace rbq {

// The launch of a stage-3 kernel K of one workgroup of kRangeThreads per query (k_range.hip, k_range_exact.hip): the probe, the
// LDS limit (one cache per K), and timing events or none.
template <auto K, class Params>
hipError_t launch_range_kernel(const Params& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    static LdsAttrCache attr;
    if (probe_stage(3, reinterpret_cast<const void*>(K), dim3(nq), kRangeThreads, lds)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(K), lds, device);
    if (e != hipSuccess) return e;
    if (ev0) hipExtLaunchKernelGGL(K, dim3(nq), dim3(kRangeThreads), lds, s, ev0, ev1, 0, P);
    else hipLaunchKernelGGL(K, dim3(nq), dim3(kRangeThreads), lds, s, P);
    return hipGetLastError();
}

// Raw rows (set_rerank_vectors) under the exact scorers of rerank_score.hpp: 16-byte loads go to 4-byte aligned addresses only.
// 16-bit rows all start on one exactly when the base does and dim is even; otherwise the scorer loads element by element (the
// slow path; callers who care pad dim to even).  The value of the params' raw_by_element.
inline uint32_t raw_rows_by_element(const void* raw, int raw_dtype, uint32_t dim) {
    return raw_dtype != kRawF32 && ((dim & 1u) != 0u || (reinterpret_cast<uintptr_t>(raw) & 3u) != 0u) ? 1u : 0u;
}
// The runtime raw_dtype as a template argument: f(std::integral_constant<int, kRawF32 / kRawF16 / kRawBf16>).
template <class F>
hipError_t dispatch_raw_dtype(int raw_dtype, F f) {
    if (raw_dtype == kRawF32) return f(std::integral_constant<int, kRawF32>{});
    if (raw_dtype == kRawF16) return f(std::integral_constant<int, kRawF16>{});
    if (raw_dtype == kRawBf16) return f(std::integral_constant<int, kRawBf16>{});
    return hipErrorInvalidValue;
}

} // namespace rbq
