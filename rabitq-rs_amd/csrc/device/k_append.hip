// k_append.hip — device side of rbq_index_append: the carry of an index into the geometry of a grown one,
// the id bound of a handle, and the nearest-list assignment of rotated rows (KmGemmAssign, km_common.hpp).  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "launch.hpp"
#include "km_common.hpp"
#include "../host/rbq_append_plan.hpp"

namespace rbq {

// 16 bytes of a per-slot f32 array: carried, or the zero fill
__device__ __forceinline__ void carry_unit(const float* s, float* d, size_t si, size_t di, bool has) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (has) v = reinterpret_cast<const uint4*>(s)[si];
    reinterpret_cast<uint4*>(d)[di] = v;
}

// One workgroup per block of the grown index (grid-stride).  The block's record and its 32 ex codes are one run of 16-byte units
// that the 256 lanes walk together: a wave instruction moves 1 KiB of contiguous bytes, whole 128-byte lines (both strides are
// multiples of 128).  The five per-slot arrays are 256 + 4 x 128 bytes per block: 48 lanes of the last wave take one unit each,
// and 8 more the residual norms of an MSTG handle (128 bytes per block; null for an IVF handle).
// A block without a source gets the streamed builder's fill.  Bandwidth-bound: no LDS, nothing kept between blocks.
__global__ __launch_bounds__(256) void k_append_carry(AppendCarryParams P) {
    const uint32_t tid = threadIdx.x;
    const uint32_t tot16 = P.rec16 + P.ex16;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u), ones = make_uint4(~0u, ~0u, ~0u, ~0u);
    for (uint32_t b = blockIdx.x; b < P.nb_new; b += gridDim.x) {
        const uint32_t c = P.block_list[b];
        uint32_t sb = rbq_host::append_src_block(b, P.gb0_new[c], P.gb0_old[c], P.n_old[c]);
        if (sb >= P.nb_old) sb = rbq_host::kAppendNoBlock; // (never for a plan that matches the old index)
        const bool has = sb != rbq_host::kAppendNoBlock; // uniform
        const uint4* rs = reinterpret_cast<const uint4*>(P.src.blocks) + (size_t)(has ? sb : 0u) * P.rec16;
        const uint4* es = reinterpret_cast<const uint4*>(P.src.ex) + (size_t)(has ? sb : 0u) * P.ex16;
        uint4* rd = reinterpret_cast<uint4*>(P.dst.blocks) + (size_t)b * P.rec16;
        uint4* ed = reinterpret_cast<uint4*>(P.dst.ex) + (size_t)b * P.ex16;
        for (uint32_t i = tid; i < tot16; i += 256u) {
            const bool rec = i < P.rec16;
            uint4 v = zero;
            if (has) v = rec ? rs[i] : es[i - P.rec16];
            if (rec) rd[i] = v;
            else ed[i - P.rec16] = v;
        }
        if (tid >= 192u) {
            const uint32_t l = tid - 192u;
            if (l < 16u) { // ids: 16 units
                const uint4* s = reinterpret_cast<const uint4*>(P.src.ids) + (size_t)(has ? sb : 0u) * 16u + l;
                uint4 v = ones; // (not `has ? *s : ones`: the compiler then selects between addresses and parks `ones` in scratch)
                if (has) v = *s;
                reinterpret_cast<uint4*>(P.dst.ids)[(size_t)b * 16u + l] = v;
            } else if (l < 48u) { // fadd_ex, fres_ex, delta, vl: 8 units each (branches, not a pointer table: no scratch)
                const uint32_t a = (l - 16u) >> 3, u = (l - 16u) & 7u;
                const size_t si = (size_t)(has ? sb : 0u) * 8u + u, di = (size_t)b * 8u + u;
                if (a == 0u) { if (P.dst.fadd) carry_unit(P.src.fadd, P.dst.fadd, si, di, has); }
                else if (a == 1u) { if (P.dst.fres) carry_unit(P.src.fres, P.dst.fres, si, di, has); }
                else if (a == 2u) carry_unit(P.src.delta, P.dst.delta, si, di, has);
                else carry_unit(P.src.vl, P.dst.vl, si, di, has);
            } else if (l < 56u) { // rnorm (MSTG handles): 8 units, the next lanes of the same wave
                const uint32_t u = l - 48u;
                if (P.dst.rnorm) carry_unit(P.src.rnorm, P.dst.rnorm, (size_t)(has ? sb : 0u) * 8u + u, (size_t)b * 8u + u, has);
            }
        }
    }
}

// max over the real slots of id + 1 (an id of 2^64 - 1 saturates)
__global__ __launch_bounds__(256) void k_append_id_bound(const uint64_t* __restrict__ ids, const uint32_t* __restrict__ block_nv,
                                                         uint64_t n_slots, unsigned long long* __restrict__ out) {
    unsigned long long m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * 256u) {
        if ((uint32_t)(i & 31u) < block_nv[i >> 5]) {
            const unsigned long long id = ids[i], v = id + 1ull ? id + 1ull : id;
            m = v > m ? v : m;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(out, m);
}

hipError_t launch_append_carry(const AppendCarryParams& P, int device, hipStream_t s) {
    if (!P.nb_new) return hipSuccess;
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e) return e;
    const uint32_t grid = std::min<uint32_t>(P.nb_new, (uint32_t)std::max(cus, 1) * 8u); // every CU busy, the rest by the stride
    hipLaunchKernelGGL(k_append_carry, dim3(grid), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_append_id_bound(const uint64_t* ids, const uint32_t* block_nv, uint64_t n_blocks, unsigned long long* out, hipStream_t s) {
    if (!n_blocks) return hipSuccess;
    const uint64_t n_slots = n_blocks * 32u;
    hipLaunchKernelGGL(k_append_id_bound, dim3((unsigned)std::min<uint64_t>(2048, grid_of(n_slots, 256))), dim3(256), 0, s, ids, block_nv,
                       n_slots, out);
    return hipGetLastError();
}

struct AppendAssign {
    KmTemp t;
    KmGemmAssign g;
    float* nx = nullptr; // [rows] canonical norms of the rotated rows
    uint64_t rows = 0;
};

hipError_t append_assign_create(uint64_t rows, uint64_t k, uint32_t D, int device, AppendAssign** out) {
    AppendAssign* a = new (std::nothrow) AppendAssign();
    if (!a) return hipErrorOutOfMemory;
    a->rows = rows;
    hipError_t e = a->g.alloc(a->t, rows, k, D, device, 0);
    if (!e) e = a->t.alloc(&a->nx, rows);
    if (e) { delete a; return e; }
    *out = a;
    return hipSuccess;
}

hipError_t append_assign_run(AppendAssign* a, const float* rows, uint32_t n, const float* cent, uint32_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    if (n > a->rows) return hipErrorInvalidValue;
    hipError_t e = launch_row_norms(rows, n, a->g.cv.dim, a->nx, s);
    return e ? e : a->g.run(rows, a->nx, n, cent, out, nullptr, s);
}

void append_assign_free(AppendAssign* a) { delete a; }

} // namespace rbq
