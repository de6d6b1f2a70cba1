// k_fetch.hip — translation unit of fetch_embedding (rbq_index_fetch_embeddings, include/rbq.h; the crate's
// IvfRabitqIndex::fetch_embedding, src/ivf.rs:1247-1307).  gfx950 only.
//
//   k_fetch_gather  the id map's input: (id, slot) of every real slot in (cluster, position) order, pad slots dropped
//   (sort)          rocprim's stable radix sort by id: of equal ids the first in (cluster, position) order stays first
//   k_fetch_vec     one workgroup per requested id: lower-bound search in the map, then the codes (unpack_single_vector,
//                   unpack_ex_code), the rotated vector (centroid + delta * code) + vl, and for FHT-Kac the inverse rotation
//                   in LDS (inverse_rotate_into, src/rotation.rs:403-480) -> the output row.  For the Matrix rotator it
//                   writes the rotated row to a scratch row instead.
//   k_fetch_matrix  Matrix rotator: out[v][col] = sum over rows r of R[r][col] * rot[v][r] (src/rotation.rs:175-196) as a
//                   tiled VALU kernel; every output is one serial chain over r = 0, 1, ... from 0.0f, multiply and add apart
//
// Every float operation is the crate's, one at a time and in its order (-ffp-contract=off keeps mul and add apart); the
// reciprocals 1 / fac and 1 / n are the crate's f32 divisions, done on the host.
#include <hip/hip_runtime.h>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "launch.hpp"
#include "kernels.hpp"
#include "codes.hpp"
#include "fetch.hpp"

namespace rbq {

namespace {

__global__ __launch_bounds__(256) void k_fetch_gather(const uint64_t* __restrict__ vstart, const uint32_t* __restrict__ list_gb0,
                                                      uint32_t n_lists, const uint64_t* __restrict__ slot_ids, uint64_t n_vectors,
                                                      uint64_t* __restrict__ ids_out, uint32_t* __restrict__ slots_out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vectors; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_lists; // largest c with vstart[c] <= i: a list that holds entry i (empty lists share its start)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (vstart[mid] <= i) lo = mid; else hi = mid;
        }
        const uint32_t slot = list_gb0[lo] * 32u + (uint32_t)(i - vstart[lo]);
        ids_out[i] = slot_ids[slot];
        slots_out[i] = slot;
    }
}

// lower bound of `id` in the map: the first (cluster, position) occurrence
__device__ __forceinline__ bool fetch_lookup(const FetchParams& P, uint64_t id, uint32_t& slot) {
    uint64_t lo = 0, hi = P.n_map;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (P.map_ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (lo < P.n_map && P.map_ids[lo] == id) { slot = P.map_slots[lo]; return true; }
    return false;
}

// rotated reconstruction of dimension i of `slot` (fetch_embedding steps 1-3)
__device__ __forceinline__ float fetch_recon(const FetchParams& P, const uint8_t* __restrict__ blk, const uint8_t* __restrict__ exs,
                                             const float* __restrict__ cent, uint32_t v, float delta, float vl, uint32_t i) {
    const uint32_t bit = (dev_code_byte(blk, P.Dc >> 7, i >> 3, v) >> (7u - (i & 7u))) & 1u;
    const uint32_t ex = P.ex_bits ? dev_ex_code(exs, P.cpu, P.ex_bits, i) : 0u;
    const uint32_t code = ex + (bit << P.ex_bits);
    const float t = cent[i] + delta * (float)code;
    return t + vl;
}

template <bool kMatrix>
__global__ __launch_bounds__(kFetchThreads) void k_fetch_vec(FetchParams P, const uint64_t* __restrict__ ids, uint64_t n,
                                                             float* __restrict__ out, uint8_t* __restrict__ found,
                                                             float* __restrict__ rows) {
    __shared__ float s[kMatrix ? 1 : kFetchMaxD];
    __shared__ uint32_t s_slot, s_list, s_hit;
    const uint32_t D = P.D, dim = P.dim, tid = threadIdx.x;
    const size_t stride = (size_t)P.Dc * 4 + 384;
    for (uint64_t q = blockIdx.x; q < n; q += gridDim.x) {
        if (tid == 0) {
            uint32_t slot = 0, c = 0;
            const bool hit = fetch_lookup(P, ids[q], slot);
            if (hit) { // largest c with list_gb0[c] <= block (an empty list shares the first block of the next one)
                uint32_t lo = 0, hi = P.n_lists;
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (P.list_gb0[mid] <= (slot >> 5)) lo = mid; else hi = mid;
                }
                c = lo;
            }
            s_slot = slot; s_list = c; s_hit = hit;
            found[q] = hit ? 1 : 0;
        }
        __syncthreads();
        const uint32_t slot = s_slot, c = s_list;
        const bool hit = s_hit != 0;
        __syncthreads(); // (s_slot / s_list / s_hit are rewritten by the next id)
        if (kMatrix) {
            float* row = rows + q * D;
            if (!hit) {
                for (uint32_t i = tid; i < D; i += blockDim.x) row[i] = 0.0f;
                continue;
            }
            const uint8_t* blk = P.blocks + (size_t)(slot >> 5) * stride;
            const uint8_t* exs = P.ex + (size_t)slot * P.exd;
            const float* cent = P.centroids + (size_t)c * D;
            const float delta = P.delta[slot], vl = P.vl[slot];
            for (uint32_t i = tid; i < D; i += blockDim.x) row[i] = fetch_recon(P, blk, exs, cent, slot & 31u, delta, vl, i);
            continue;
        }
        float* o = out + q * dim;
        if (!hit) {
            for (uint32_t i = tid; i < dim; i += blockDim.x) o[i] = 0.0f;
            continue;
        }
        {
            const uint8_t* blk = P.blocks + (size_t)(slot >> 5) * stride;
            const uint8_t* exs = P.ex + (size_t)slot * P.exd;
            const float* cent = P.centroids + (size_t)c * D;
            const float delta = P.delta[slot], vl = P.vl[slot];
            for (uint32_t i = tid; i < D; i += blockDim.x) s[i] = fetch_recon(P, blk, exs, cent, slot & 31u, delta, vl, i);
            __syncthreads();
        }
        lds_inverse_fht_kac(s, D, P.trunc, P.rfac, P.rlen, P.rot_blob);
        for (uint32_t i = tid; i < dim; i += blockDim.x) o[i] = s[i];
        __syncthreads(); // s is rewritten by the next id
    }
}

// Matrix rotator: a 64 x 64 tile of (vectors, columns) per workgroup, 4 x 4 outputs per thread; the k loop walks the rows of R
// in order, 16 at a time through LDS, so each output's chain is the serial one.  D % 16 == 0 (validate_header): every k step is whole.
constexpr uint32_t kMatT = 64, kMatK = 16;
__global__ __launch_bounds__(256) void k_fetch_matrix(const float* __restrict__ R, const float* __restrict__ rows, const uint8_t* __restrict__ found,
                                                      uint64_t n, uint32_t D, uint32_t dim, float* __restrict__ out) {
    __shared__ float xs[kMatK][kMatT + 1]; // xs[k][v]
    __shared__ float rs[kMatK][kMatT];     // rs[k][col]
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint64_t v0 = (uint64_t)blockIdx.x * kMatT;
    const uint32_t c0 = blockIdx.y * kMatT;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    for (uint32_t k0 = 0; k0 < D; k0 += kMatK) {
#pragma unroll
        for (uint32_t e = tid; e < kMatK * kMatT; e += 256) {
            const uint32_t vv = e >> 4, kk = e & 15u; // rows: 16 consecutive k of one vector
            const uint64_t v = v0 + vv;
            xs[kk][vv] = v < n ? rows[v * D + k0 + kk] : 0.0f;
            const uint32_t rk = e >> 6, cc = e & 63u;  // R: 64 consecutive columns of one row
            rs[rk][cc] = c0 + cc < dim ? R[(size_t)(k0 + rk) * D + c0 + cc] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t kk = 0; kk < kMatK; ++kk) {
            float x[4], r[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) x[a] = xs[kk][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) r[b] = rs[kk][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float p = r[b] * x[a];
                    acc[a][b] = acc[a][b] + p;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint64_t v = v0 + ty + 16 * a;
        if (v >= n) continue;
        const bool hit = found[v] != 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t col = c0 + tx + 16 * b;
            if (col < dim) out[v * dim + col] = hit ? acc[a][b] : 0.0f;
        }
    }
}

} // namespace

hipError_t launch_fetch_gather(const uint64_t* vstart, const uint32_t* list_gb0, uint32_t n_lists, const uint64_t* slot_ids,
                               uint64_t n_vectors, uint64_t* ids_out, uint32_t* slots_out, hipStream_t s) {
    if (!n_vectors) return hipSuccess;
    const uint64_t blocks = (n_vectors + 255) / 256;
    hipLaunchKernelGGL(k_fetch_gather, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, vstart, list_gb0, n_lists,
                       slot_ids, n_vectors, ids_out, slots_out);
    return hipGetLastError();
}

hipError_t sort_pairs_u64_u32(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in,
                              uint32_t* vals_out, size_t n, hipStream_t s) {
    return rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, 64u, s);
}

hipError_t launch_fetch(const FetchParams& P, const uint64_t* ids, uint64_t n, float* out, uint8_t* found, float* rows,
                        hipStream_t s) {
    if (!n) return hipSuccess;
    if (P.D > kFetchMaxD || P.D == 0) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(n < (1u << 18) ? n : (1u << 18));
    if (P.rotator == 1) { // RBQ_ROTATOR_FHT_KAC
        hipLaunchKernelGGL(k_fetch_vec<false>, dim3(grid), dim3(kFetchThreads), 0, s, P, ids, n, out, found, nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_fetch_vec<true>, dim3(grid), dim3(kFetchThreads), 0, s, P, ids, n, out, found, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_fetch_matrix((const float*)P.rot_blob, rows, found, n, P.D, P.dim, out, s);
}

hipError_t launch_fetch_matrix(const float* R, const float* rows, const uint8_t* found, uint64_t n, uint32_t D, uint32_t dim, float* out,
                               hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t gx = (n + kMatT - 1) / kMatT;
    if (gx > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fetch_matrix, dim3((uint32_t)gx, (dim + kMatT - 1) / kMatT), dim3(256), 0, s, R, rows, found, n, D, dim, out);
    return hipGetLastError();
}

} // namespace rbq
