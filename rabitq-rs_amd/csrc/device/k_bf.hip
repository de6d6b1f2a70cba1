// k_bf.hip — translation unit of the brute-force index's kernels (bf.hpp) and their launchers.  gfx950 only.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "bf.hpp"

namespace rbq {

hipError_t launch_bf_dist(const BfDistParams& p, hipStream_t s) {
    const dim3 grid((uint32_t)((p.nv + kBfVec - 1) / kBfVec), (p.nq + kBfQ - 1) / kBfQ);
    if (p.ex_bits == 6) hipLaunchKernelGGL(k_bf_dist<6>, grid, dim3(kBfVec), 0, s, p);
    else if (p.ex_bits == 2) hipLaunchKernelGGL(k_bf_dist<2>, grid, dim3(kBfVec), 0, s, p);
    else hipLaunchKernelGGL(k_bf_dist<0>, grid, dim3(kBfVec), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_bf_select(const BfSelectParams& p, hipStream_t s) {
    static LdsAttrCache attr;
    const size_t lds = p.lds_heap ? ((size_t)p.top_k + 1) * 8 : 0;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = attr.ensure(reinterpret_cast<const void*>(&k_bf_select), lds, dev);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bf_select, dim3(p.nq), dim3(64), lds, s, p);
    return hipGetLastError();
}

} // namespace rbq
