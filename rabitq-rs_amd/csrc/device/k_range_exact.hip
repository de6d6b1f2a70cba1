// k_range_exact.hip — translation unit of the exact range scan (range.hpp: k_range<0, 0, V, XR, XIP>; options range_exact /
// range_exact_radius_bits) and its launcher.  gfx950 only.  The runtime-dimension kernel per numeric variant,
// raw element and metric: 18 instantiations.  The estimate-only instantiations stay in k_range.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "launch.hpp"

#pragma clang fp contract(off)

#include "range.hpp" // (after the pragma: the exact scorer's sums are unfused)

namespace rbq {
namespace {

template <int V, int XR, bool XIP>
hipError_t launch_rx(const RangeExactParams& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    static LdsAttrCache attr;
    if (probe_stage(3, reinterpret_cast<const void*>(&k_range<0, 0, V, XR, XIP>), dim3(nq), kRangeThreads, lds)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_range<0, 0, V, XR, XIP>), lds, device);
    if (e != hipSuccess) return e;
    if (ev0) hipExtLaunchKernelGGL((k_range<0, 0, V, XR, XIP>), dim3(nq), dim3(kRangeThreads), lds, s, ev0, ev1, 0, P);
    else hipLaunchKernelGGL((k_range<0, 0, V, XR, XIP>), dim3(nq), dim3(kRangeThreads), lds, s, P);
    return hipGetLastError();
}
template <int V, int XR>
hipError_t launch_rx_m(const RangeExactParams& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return P.metric == 1u ? launch_rx<V, XR, true>(P, nq, lds, device, s, ev0, ev1) : launch_rx<V, XR, false>(P, nq, lds, device, s, ev0, ev1);
}
template <int V>
hipError_t launch_rx_v(const RangeExactParams& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (P.raw_dtype == kRawF32) return launch_rx_m<V, kRawF32>(P, nq, lds, device, s, ev0, ev1);
    if (P.raw_dtype == kRawF16) return launch_rx_m<V, kRawF16>(P, nq, lds, device, s, ev0, ev1);
    if (P.raw_dtype == kRawBf16) return launch_rx_m<V, kRawBf16>(P, nq, lds, device, s, ev0, ev1);
    return hipErrorInvalidValue;
}

} // namespace

hipError_t launch_range_exact(const RangeExactParams& P0, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    RangeExactParams P = P0;
    if (P.dim == 0u || P.n_raw == 0u || !P.raw) return hipErrorInvalidValue; // (row 0 stands in for a missing row: it must exist)
    const size_t lds = range_exact_lds_bytes(P.Dc, P.D, P.ex_bits, P.dim);
    if (lds > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    // as launch_rerank_pool: 16-byte loads go to 4-byte aligned addresses only
    P.raw_by_element = P.raw_dtype != kRawF32 && ((P.dim & 1u) != 0u || (reinterpret_cast<uintptr_t>(P.raw) & 3u) != 0u) ? 1u : 0u;
    if (P.numeric_variant == (uint32_t)kVarAvx512) return launch_rx_v<kVarAvx512>(P, nq, lds, device, s, ev0, ev1);
    if (P.numeric_variant == (uint32_t)kVarAvx2) return launch_rx_v<kVarAvx2>(P, nq, lds, device, s, ev0, ev1);
    if (P.numeric_variant == (uint32_t)kVarPortable) return launch_rx_v<kVarPortable>(P, nq, lds, device, s, ev0, ev1);
    return hipErrorInvalidValue;
}

} // namespace rbq
