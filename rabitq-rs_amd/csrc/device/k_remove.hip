// k_remove.hip — device side of rbq_index_remove_ids: the keep mask of every block of an index against a
// sorted set of ids, the kept count of every list, the slot map of the shrunk index and the gather of every array through it.
// gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "launch.hpp"
#include "../host/rbq_remove_plan.hpp"
#include <rocprim/rocprim.hpp>

namespace rbq {

namespace {

struct PopcountOp {
    __host__ __device__ uint32_t operator()(uint32_t m) const { return (uint32_t)__builtin_popcount(m); }
};

// One lane per old slot, a wave over two blocks.  A slot stays when it is real (below its block's vector count) and its id is not
// in the sorted set: a lower bound per slot, so every occurrence of a stored id is found.  mask[b] bit v = lane v of block b stays.
__global__ __launch_bounds__(256) void k_remove_mark(const uint64_t* __restrict__ ids, const uint32_t* __restrict__ block_nv,
                                                     uint64_t n_slots, const uint64_t* __restrict__ set, uint64_t n_set,
                                                     uint32_t* __restrict__ mask) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; (i & ~63ull) < n_slots; i += stride) { // (uniform per wave)
        bool keep = false;
        if (i < n_slots && (uint32_t)(i & 31u) < block_nv[i >> 5]) {
            const uint64_t id = ids[i];
            uint64_t lo = 0, hi = n_set;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (set[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            keep = !(lo < n_set && set[lo] == id);
        }
        const unsigned long long bal = __ballot(keep);
        if (i < n_slots && (i & 31u) == 0) mask[i >> 5] = (uint32_t)((i & 32u) ? bal >> 32 : bal);
    }
}

// kept[c] = survivors of list c, from the exclusive scan of the per-block kept counts (scan [n_blocks + 1])
__global__ __launch_bounds__(256) void k_remove_list_kept(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ gb0_old,
                                                          const uint32_t* __restrict__ n_old, uint32_t n_lists, uint32_t n_blocks,
                                                          uint32_t* __restrict__ kept) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_lists) return;
    const uint32_t b0 = gb0_old[c], b1 = b0 + (n_old[c] + 31u) / 32u;
    kept[c] = (b0 <= n_blocks && b1 <= n_blocks) ? scan[b1] - scan[b0] : 0xffffffffu; // (never: the handle's tables agree)
}

// map[new slot] = old slot, for every kept old slot (the pads keep the caller's fill of all ones)
__global__ __launch_bounds__(256) void k_remove_slot_map(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ scan,
                                                         const uint32_t* __restrict__ block_list_old, const uint32_t* __restrict__ gb0_old,
                                                         const uint32_t* __restrict__ gb0_new, uint64_t n_slots_old, uint64_t n_slots_new,
                                                         uint32_t* __restrict__ map) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_slots_old; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t b = (uint32_t)(i >> 5), lane = (uint32_t)(i & 31u), m = mask[b];
        if (!((m >> lane) & 1u)) continue;
        const uint32_t c = block_list_old[b];
        const uint32_t dst = rbq_host::remove_dst_slot(gb0_new[c], rbq_host::remove_rank(scan[b], scan[gb0_old[c]], m, lane));
        if (dst < n_slots_new) map[dst] = (uint32_t)i;
    }
}

// One per-slot f32 value: gathered, or the zero fill
__device__ __forceinline__ void gather_f32(const float* s, float* d, uint32_t src, size_t dst, bool has) {
    float x = 0.0f;
    if (has) x = s[src];
    d[dst] = x;
}

// One workgroup per block of the shrunk index (grid-stride).  Lane v = tid % 32 of every half wave serves new lane v: it reads
// its source slot from the map once and walks the code granules tid / 32, + 8, ... from the source block's lane to its own, 16
// bytes each, so a wave instruction stores 1 KiB of contiguous bytes and loads contiguous bytes wherever a run of survivors is.
// The 8-byte tail granule, the three factor rows and the five per-slot arrays are per-lane gathers spread over the eight half
// waves (half waves 0-4 the slot arrays, 5-7 the factor rows; half wave 5 also the residual norms of an MSTG handle, a sixth
// slot array that an IVF handle does not have).  The ex codes of a slot are contiguous: 8 lanes per slot copy them 128 bytes at a time (the source slot comes from the
// lane that holds it, by a shuffle).  A pad lane gets the builder's fill: zeros, and an id of all ones.  Bandwidth-bound: no LDS,
// nothing kept between blocks.
__global__ __launch_bounds__(256) void k_remove_gather(RemoveGatherParams P) {
    const uint32_t tid = threadIdx.x, v = tid & 31u, grp = tid >> 5;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t code_bytes = P.rec - 384u;
    for (uint32_t b = blockIdx.x; b < P.nb_new; b += gridDim.x) {
        uint32_t src = P.map[(size_t)b * 32u + v];
        if (src >= P.n_slots_old) src = rbq_host::kRemoveNoSlot; // (a pad; never anything else for a map of this index)
        const bool has = src != rbq_host::kRemoveNoSlot;
        const uint32_t sb = has ? src >> 5 : 0u, sl = has ? src & 31u : 0u;
        const uint8_t* rs = P.src.blocks + (size_t)sb * P.rec;
        uint8_t* rd = P.dst.blocks + (size_t)b * P.rec;
        for (uint32_t g = grp; g < P.G16; g += 8u) {
            uint4 x = zero;
            if (has) x = *reinterpret_cast<const uint4*>(rs + (size_t)g * 512u + sl * 16u);
            *reinterpret_cast<uint4*>(rd + (size_t)g * 512u + v * 16u) = x;
        }
        if (P.tail && grp == (P.G16 & 7u)) { // the half granule of Dc % 128 == 64: the next half wave in turn
            uint2 x = make_uint2(0u, 0u);
            if (has) x = *reinterpret_cast<const uint2*>(rs + (size_t)P.G16 * 512u + sl * 8u);
            *reinterpret_cast<uint2*>(rd + (size_t)P.G16 * 512u + v * 8u) = x;
        }
        if (grp >= 5u) { // f_add | f_rescale | f_error
            const uint32_t off = code_bytes + (7u - grp) * 128u;
            uint32_t x = 0u;
            if (has) x = *reinterpret_cast<const uint32_t*>(rs + off + sl * 4u);
            *reinterpret_cast<uint32_t*>(rd + off + v * 4u) = x;
        }
        const size_t ds = (size_t)b * 32u + v;
        if (grp == 0u) { // (branches, not a pointer table: no scratch)
            uint64_t x = ~0ull;
            if (has) x = P.src.ids[src];
            P.dst.ids[ds] = x;
        } else if (grp == 1u) { if (P.dst.fadd) gather_f32(P.src.fadd, P.dst.fadd, src, ds, has); }
        else if (grp == 2u) { if (P.dst.fres) gather_f32(P.src.fres, P.dst.fres, src, ds, has); }
        else if (grp == 3u) gather_f32(P.src.delta, P.dst.delta, src, ds, has);
        else if (grp == 4u) gather_f32(P.src.vl, P.dst.vl, src, ds, has);
        else if (grp == 5u) { if (P.dst.rnorm) gather_f32(P.src.rnorm, P.dst.rnorm, src, ds, has); } // (its second task, after a factor row)
        if (P.ex16) { // slot tid / 8 of the block, unit tid % 8, + 8, ...; lane (slot % 32) of this wave holds the slot's source
            const uint32_t slot = tid >> 3, j = tid & 7u;
            const uint32_t s2 = (uint32_t)__shfl((int)src, (int)(slot & 31u));
            const bool has2 = s2 != rbq_host::kRemoveNoSlot;
            const uint4* es = reinterpret_cast<const uint4*>(P.src.ex) + (size_t)(has2 ? s2 : 0u) * P.ex16;
            uint4* ed = reinterpret_cast<uint4*>(P.dst.ex) + ((size_t)b * 32u + slot) * P.ex16;
            for (uint32_t u = j; u < P.ex16; u += 8u) {
                uint4 x = zero;
                if (has2) x = es[u];
                ed[u] = x;
            }
        }
    }
}

} // namespace

hipError_t sort_keys_u64(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, size_t n, hipStream_t s) {
    return rocprim::radix_sort_keys(tmp, *tmp_bytes, keys_in, keys_out, n, 0u, 64u, s);
}

hipError_t launch_remove_mark(const uint64_t* ids, const uint32_t* block_nv, uint64_t n_blocks, const uint64_t* set, uint64_t n_set,
                              uint32_t* mask, hipStream_t s) {
    if (!n_blocks) return hipSuccess;
    const uint64_t n_slots = n_blocks * 32u;
    hipLaunchKernelGGL(k_remove_mark, dim3((unsigned)std::min<uint64_t>(8192, (n_slots + 255u) / 256u)), dim3(256), 0, s, ids, block_nv,
                       n_slots, set, n_set, mask);
    return hipGetLastError();
}

hipError_t remove_scan_kept(void* tmp, size_t* tmp_bytes, const uint32_t* mask, uint32_t* scan, uint64_t n, hipStream_t s) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, rocprim::make_transform_iterator(mask, PopcountOp()), scan, 0u, (size_t)n,
                                   rocprim::plus<uint32_t>(), s);
}

hipError_t launch_remove_list_kept(const uint32_t* scan, const uint32_t* gb0_old, const uint32_t* n_old, uint32_t n_lists,
                                   uint64_t n_blocks, uint32_t* kept, hipStream_t s) {
    if (!n_lists) return hipSuccess;
    hipLaunchKernelGGL(k_remove_list_kept, dim3((n_lists + 255u) / 256u), dim3(256), 0, s, scan, gb0_old, n_old, n_lists,
                       (uint32_t)n_blocks, kept);
    return hipGetLastError();
}

hipError_t launch_remove_slot_map(const uint32_t* mask, const uint32_t* scan, const uint32_t* block_list_old, const uint32_t* gb0_old,
                                  const uint32_t* gb0_new, uint64_t nb_old, uint64_t nb_new, uint32_t* map, hipStream_t s) {
    if (!nb_old || !nb_new) return hipSuccess;
    const uint64_t n_slots = nb_old * 32u;
    hipLaunchKernelGGL(k_remove_slot_map, dim3((unsigned)std::min<uint64_t>(8192, (n_slots + 255u) / 256u)), dim3(256), 0, s, mask, scan,
                       block_list_old, gb0_old, gb0_new, n_slots, nb_new * 32u, map);
    return hipGetLastError();
}

hipError_t launch_remove_gather(const RemoveGatherParams& P, int device, hipStream_t s) {
    if (!P.nb_new) return hipSuccess;
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e) return e;
    const uint32_t grid = std::min<uint32_t>(P.nb_new, (uint32_t)std::max(cus, 1) * 8u); // every CU busy, the rest by the stride
    hipLaunchKernelGGL(k_remove_gather, dim3(grid), dim3(256), 0, s, P);
    return hipGetLastError();
}

} // namespace rbq
