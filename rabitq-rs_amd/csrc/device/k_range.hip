// k_range.hip — translation unit of the range search's scan (range.hpp) and its launcher.  gfx950 only.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "launch.hpp"
#include "range.hpp"

namespace rbq {
namespace {

template <int DT, int EX, int V = kVarAvx512>
hipError_t launch_range_r(const RangeParams& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    static LdsAttrCache attr;
    if (probe_stage(3, reinterpret_cast<const void*>(&k_range<DT, EX, V>), dim3(nq), kRangeThreads, lds)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_range<DT, EX, V>), lds, device);
    if (e != hipSuccess) return e;
    if (ev0) hipExtLaunchKernelGGL((k_range<DT, EX, V>), dim3(nq), dim3(kRangeThreads), lds, s, ev0, ev1, 0, P);
    else hipLaunchKernelGGL((k_range<DT, EX, V>), dim3(nq), dim3(kRangeThreads), lds, s, P);
    return hipGetLastError();
}
template <int DT>
hipError_t launch_range_d(const RangeParams& P, uint32_t nq, size_t lds, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    switch (P.ex_bits) {
        case 0: return launch_range_r<DT, 0>(P, nq, lds, device, s, ev0, ev1);
        case 2: return launch_range_r<DT, 2>(P, nq, lds, device, s, ev0, ev1);
        default: return launch_range_r<DT, 6>(P, nq, lds, device, s, ev0, ev1);
    }
}

} // namespace

hipError_t launch_range(const RangeParams& P, uint32_t nq, int device, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const uint32_t D = P.D, Dc = P.Dc;
    const size_t lds = range_lds_bytes(Dc, D, P.ex_bits);
    if (P.numeric_variant != (uint32_t)kVarAvx512) { // the other numeric variants: runtime-dimension instantiations only
        if (P.numeric_variant == (uint32_t)kVarAvx2) return launch_range_r<0, 0, kVarAvx2>(P, nq, lds, device, s, ev0, ev1);
        if (P.numeric_variant == (uint32_t)kVarPortable) return launch_range_r<0, 0, kVarPortable>(P, nq, lds, device, s, ev0, ev1);
        return hipErrorInvalidValue;
    }
    if (D == Dc && D == 960) return launch_range_d<960>(P, nq, lds, device, s, ev0, ev1);
    if (D == Dc && D == 768) return launch_range_d<768>(P, nq, lds, device, s, ev0, ev1);
    if (D == Dc && D == 128) return launch_range_d<128>(P, nq, lds, device, s, ev0, ev1);
    return launch_range_r<0, 0>(P, nq, lds, device, s, ev0, ev1); // any other dimension: runtime dimension and ex_bits
}

} // namespace rbq
