// k_bf_mutate.hip — device side of rbq_bf_remove_ids and rbq_bf_fetch_embeddings (include/rbq_bf_mutate.h).
// gfx950 only.
//
//   k_bf_mark       scatters the set into a keep mask: ids are positions, so no sort and no search
//   (scan)          rocprim's exclusive scan of the mask: the rank of every survivor
//   k_bf_row_map    map[rank] = old row, for every survivor
//   k_bf_gather     every flat array of the index through the map: sign codes, ex codes, the eight factor arrays
//   k_bf_fetch_vec  one workgroup per requested id: code = ex + (bit << ex_bits) from the flat rows, the rotated vector
//                   (0.0f + delta * code) + vl, and for FHT-Kac the inverse rotation in LDS (fetch.hpp) -> the output row; for the
//                   Matrix rotator the rotated row goes to a scratch row that k_fetch_matrix (k_fetch.hip) turns back
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "launch.hpp"
#include "codes.hpp"
#include "fetch.hpp"

namespace rbq {

namespace {

struct KeepOp {
    __host__ __device__ uint32_t operator()(uint8_t k) const { return k ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void k_bf_mark(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t n, uint8_t* __restrict__ keep) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n_ids; j += (uint64_t)gridDim.x * 256u) {
        const uint64_t id = ids[j];
        if (id < n) keep[id] = 0; // (repeats store the same value)
    }
}

__global__ __launch_bounds__(256) void k_bf_row_map(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ rank, uint64_t n,
                                                    uint32_t* __restrict__ map) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
        if (keep[i]) map[rank[i]] = (uint32_t)i; // rank[i] < rank[n] = the length of map
}

constexpr uint32_t kBfGatherRows = 64; // rows of one workgroup pass
constexpr uint32_t kBfGatherU = 4;     // units in flight per lane

// `nr` rows of `len` bytes, destination rows r0 .. r0 + nr - 1 from the source rows smap[0 .. nr), in units of T (sizeof(T) divides
// len and 16, so every row of both arrays is aligned to it).  The units of the nr destination rows are one contiguous run: lane l
// stores unit l, l + 256, ..., a wave instruction 64 consecutive units, and loads consecutive units wherever a row or a run of
// surviving rows continues.  kBfGatherU loads are issued before the first store.
template <class T>
__device__ __forceinline__ void bf_gather_rows(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint32_t len, uint64_t r0,
                                               uint32_t nr, const uint32_t* smap) {
    const uint32_t upr = len / (uint32_t)sizeof(T), total = nr * upr; // <= 64 * 1536 / 2
    const T* src = reinterpret_cast<const T*>(s);
    T* dst = reinterpret_cast<T*>(d) + r0 * upr;
    uint32_t e0 = threadIdx.x;
    for (; e0 + 256u * (kBfGatherU - 1u) < total; e0 += 256u * kBfGatherU) {
        T x[kBfGatherU];
#pragma unroll
        for (uint32_t u = 0; u < kBfGatherU; ++u) {
            const uint32_t e = e0 + 256u * u, r = e / upr;
            x[u] = src[(size_t)smap[r] * upr + (e - r * upr)];
        }
#pragma unroll
        for (uint32_t u = 0; u < kBfGatherU; ++u) dst[e0 + 256u * u] = x[u];
    }
    for (; e0 < total; e0 += 256u) { // the last units of the pass, one at a time
        const uint32_t r = e0 / upr;
        dst[e0] = src[(size_t)smap[r] * upr + (e0 - r * upr)];
    }
}

// the widest unit that divides the row length and 16 bytes (rows are even: padded_dim % 16 == 0)
__device__ __forceinline__ void bf_gather_section(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint32_t len, uint64_t r0,
                                                  uint32_t nr, const uint32_t* smap) {
    if (len % 16u == 0) bf_gather_rows<uint4>(s, d, len, r0, nr, smap);
    else if (len % 8u == 0) bf_gather_rows<uint2>(s, d, len, r0, nr, smap);
    else if (len % 4u == 0) bf_gather_rows<uint32_t>(s, d, len, r0, nr, smap);
    else bf_gather_rows<uint16_t>(s, d, len, r0, nr, smap);
}

// One workgroup per kBfGatherRows rows of the shrunk index (grid-stride): their source rows go to LDS once, then the sign codes,
// the ex codes and the factors follow.  Factor array k is served by half wave k: two stores of 32 consecutive floats.
// Bandwidth-bound: nothing is kept between passes.
__global__ __launch_bounds__(256) void k_bf_gather(BfGatherParams P) {
    __shared__ uint32_t smap[kBfGatherRows];
    const uint32_t tid = threadIdx.x;
    const uint64_t passes = (P.n_new + kBfGatherRows - 1) / kBfGatherRows;
    for (uint64_t b = blockIdx.x; b < passes; b += gridDim.x) {
        const uint64_t r0 = b * kBfGatherRows;
        const uint32_t nr = (uint32_t)(P.n_new - r0 < kBfGatherRows ? P.n_new - r0 : kBfGatherRows);
        __syncthreads(); // (the last pass has read smap)
        if (tid < nr) {
            const uint32_t src = P.map[r0 + tid];
            smap[tid] = src < P.n_old ? src : (uint32_t)(P.n_old - 1); // (never clamped for a map of this index)
        }
        __syncthreads();
        bf_gather_section(P.bin_s, P.bin_d, P.bin_len, r0, nr, smap);
        if (P.ex_len) bf_gather_section(P.ex_s, P.ex_d, P.ex_len, r0, nr, smap);
        const uint32_t k = tid >> 5, l = tid & 31u;
        const float* fs = nullptr;
        float* fd = nullptr;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) // (a select per constant index, not a pointer table: no scratch)
            if (k == j) { fs = P.f_s[j]; fd = P.f_d[j]; }
        float x0 = 0.0f, x1 = 0.0f;
        if (l < nr) x0 = fs[smap[l]];
        if (l + 32u < nr) x1 = fs[smap[l + 32u]];
        if (l < nr) fd[r0 + l] = x0;
        if (l + 32u < nr) fd[r0 + l + 32u] = x1;
    }
}

// rotated reconstruction of dimension i (fetch_embedding steps 1-3 against the zero centroid, each operation on its own)
__device__ __forceinline__ float bf_recon(const uint8_t* __restrict__ bin, const uint8_t* __restrict__ exr, uint32_t ex_bits, float delta,
                                          float vl, uint32_t i) {
    const uint32_t bit = ((uint32_t)bin[i >> 3] >> (7u - (i & 7u))) & 1u;
    const uint32_t ex = ex_bits ? flat_ex_code(exr, ex_bits, i) : 0u;
    const uint32_t code = ex + (bit << ex_bits);
    const float t = 0.0f + delta * (float)code;
    return t + vl;
}

template <bool kMatrix>
__global__ __launch_bounds__(kFetchThreads) void k_bf_fetch_vec(BfFetchParams P, const uint64_t* __restrict__ ids, uint64_t n,
                                                                float* __restrict__ out, uint8_t* __restrict__ found,
                                                                float* __restrict__ rows) {
    __shared__ float s[kMatrix ? 1 : kFetchMaxD];
    const uint32_t D = P.D, dim = P.dim, tid = threadIdx.x;
    const uint64_t bin_len = D / 8, ex_len = (uint64_t)D * P.ex_bits / 8;
    for (uint64_t q = blockIdx.x; q < n; q += gridDim.x) {
        const uint64_t id = ids[q]; // (the same for every thread)
        const bool hit = id < P.n_vectors;
        if (tid == 0) found[q] = hit ? 1 : 0;
        if (!hit) {
            if (kMatrix) { for (uint32_t i = tid; i < D; i += blockDim.x) rows[q * D + i] = 0.0f; }
            else { for (uint32_t i = tid; i < dim; i += blockDim.x) out[q * dim + i] = 0.0f; }
            continue;
        }
        const uint8_t* bin = P.bin + id * bin_len;
        const uint8_t* exr = P.ex + id * ex_len;
        const float delta = P.delta[id], vl = P.vl[id];
        if (kMatrix) {
            for (uint32_t i = tid; i < D; i += blockDim.x) rows[q * D + i] = bf_recon(bin, exr, P.ex_bits, delta, vl, i);
            continue;
        }
        for (uint32_t i = tid; i < D; i += blockDim.x) s[i] = bf_recon(bin, exr, P.ex_bits, delta, vl, i);
        __syncthreads();
        lds_inverse_fht_kac(s, D, P.trunc, P.rfac, P.rlen, P.rot_blob);
        for (uint32_t i = tid; i < dim; i += blockDim.x) out[q * dim + i] = s[i];
        __syncthreads(); // s is rewritten by the next id
    }
}

} // namespace

hipError_t launch_bf_mark(const uint64_t* ids, uint64_t n_ids, uint64_t n, uint8_t* keep, hipStream_t s) {
    if (!n_ids) return hipSuccess;
    hipLaunchKernelGGL(k_bf_mark, dim3((unsigned)std::min<uint64_t>(8192, (n_ids + 255u) / 256u)), dim3(256), 0, s, ids, n_ids, n, keep);
    return hipGetLastError();
}

hipError_t bf_scan_kept(void* tmp, size_t* tmp_bytes, const uint8_t* keep, uint32_t* rank, uint64_t n, hipStream_t s) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, rocprim::make_transform_iterator(keep, KeepOp()), rank, 0u, (size_t)n,
                                   rocprim::plus<uint32_t>(), s);
}

hipError_t launch_bf_row_map(const uint8_t* keep, const uint32_t* rank, uint64_t n, uint32_t* map, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_bf_row_map, dim3((unsigned)std::min<uint64_t>(8192, (n + 255u) / 256u)), dim3(256), 0, s, keep, rank, n, map);
    return hipGetLastError();
}

hipError_t launch_bf_gather(const BfGatherParams& P, int device, hipStream_t s) {
    if (!P.n_new) return hipSuccess;
    if (!P.n_old || P.bin_len % 2u || P.ex_len % 2u) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e) return e;
    const uint64_t passes = (P.n_new + kBfGatherRows - 1) / kBfGatherRows;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(passes, (uint64_t)std::max(cus, 1) * 8u); // every CU busy, the rest by the stride
    hipLaunchKernelGGL(k_bf_gather, dim3(grid), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_bf_fetch(const BfFetchParams& P, const uint64_t* ids, uint64_t n, float* out, uint8_t* found, float* rows,
                           hipStream_t s) {
    if (!n) return hipSuccess;
    if (P.D > kFetchMaxD || P.D == 0) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(n < (1u << 18) ? n : (1u << 18));
    if (P.rotator == 1) { // RBQ_ROTATOR_FHT_KAC
        hipLaunchKernelGGL(k_bf_fetch_vec<false>, dim3(grid), dim3(kFetchThreads), 0, s, P, ids, n, out, found, nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_bf_fetch_vec<true>, dim3(grid), dim3(kFetchThreads), 0, s, P, ids, n, out, found, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_fetch_matrix((const float*)P.rot_blob, rows, found, n, P.D, P.dim, out, s);
}

} // namespace rbq
