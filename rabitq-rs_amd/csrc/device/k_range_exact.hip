// k_range_exact.hip — translation unit of the exact range scan (range.hpp: k_range<0, 0, V, XR, XIP>; options range_exact /
// range_exact_radius_bits) and its launcher.  gfx950 only.  The runtime-dimension kernel per numeric variant,
// raw element and metric: 18 instantiations.  The estimate-only instantiations stay in k_range.hip.
#include <hip/hip_runtime.h>

#include "launch_util.hpp"

#pragma clang fp contract(off)

#include "range.hpp" // (after the pragma: the exact scorer's sums are unfused)

namespace rbq {
namespace {

template <int V>
hipError_t launch_rx_v(const RangeExactParams& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return dispatch_raw_dtype(P.raw_dtype, [&](auto xr) {
        constexpr int XR = decltype(xr)::value;
        return P.metric == 1u ? launch_range_kernel<&k_range<0, 0, V, XR, true>>(P, nq, lds, device, s, ev0, ev1)
                              : launch_range_kernel<&k_range<0, 0, V, XR, false>>(P, nq, lds, device, s, ev0, ev1);
    });
}

} // namespace

hipError_t launch_range_exact(const RangeExactParams& P0, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    RangeExactParams P = P0;
    if (P.dim == 0u || P.n_raw == 0u || !P.raw) return hipErrorInvalidValue; // (row 0 stands in for a missing row: it must exist)
    const size_t lds = range_exact_lds_bytes(P.Dc, P.D, P.ex_bits, P.dim);
    if (lds > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    P.raw_by_element = raw_rows_by_element(P.raw, P.raw_dtype, P.dim);
    if (P.numeric_variant == (uint32_t)kVarAvx512) return launch_rx_v<kVarAvx512>(P, nq, lds, device, s, ev0, ev1);
    if (P.numeric_variant == (uint32_t)kVarAvx2) return launch_rx_v<kVarAvx2>(P, nq, lds, device, s, ev0, ev1);
    if (P.numeric_variant == (uint32_t)kVarPortable) return launch_rx_v<kVarPortable>(P, nq, lds, device, s, ev0, ev1);
    return hipErrorInvalidValue;
}

} // namespace rbq
