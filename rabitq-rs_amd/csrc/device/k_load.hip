// k_load.hip — translation unit of the streamed RBQ1 loader's kernels (rbq_index_load_rbq1_stream, include/rbq_persist.h).
// gfx950 only.
//
//   k_load_span      one span of the stream's cluster region -> the device layout, driven by the span's piece table
//                    (csrc/host/rbq_load_stream.hpp): one workgroup serves 256 f32s / ids / factor slots, 8 batch records or 16
//                    ex codes of ONE piece, which it finds by binary search over the pieces' first workgroups.  Per section:
//                      centroid   f32 words copied
//                      batch      k_relayout_blocks' un-interleave (relayout.hpp): one half-wave per record, lane = vector
//                      ids        two words per id; pad slots behind a list's last vector get ~0
//                      ex         the u64 length prefix is compared with exb (a wrong one: atomic minimum of its file
//                                 position) and skipped, the code re-packed lane-major as k_relayout_ex does, 16 lanes per
//                                 vector; pad slots get zero codes
//                      factors    f_add_ex, f_rescale_ex, delta, vl as words; pad slots get 0.0
//   k_load_block_nv  real vectors of every block, the table k_block_summary wants
//
// What the kernels may assume about addresses: a span starts at a field boundary and every field of an RBQ1 stream lies at a
// multiple of 4 bytes from its start, NOT 8 — ids and prefixes are read as two words or bytewise.  That much holds only for
// streams this build serves (padded_dim % 16 == 0); for any other stream the launch is check-only (scatter == 0) and the
// prefixes, the only bytes read, are read bytewise.  Every address read lies inside a piece, and the host cuts pieces inside
// the span.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "types.hpp"
#include "../host/rbq_load_stream.hpp"

namespace rbq {

namespace {

using rbq_host::LoadPiece;

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

// inverse of pack_codes (relayout.hpp: fastscan_byte_dev)
__device__ __forceinline__ uint32_t load_fastscan_byte(const uint8_t* __restrict__ packed, uint32_t col, uint32_t v) {
    const uint32_t u = v & 15u, j = 2u * (u & 7u) + (u >> 3);
    const uint32_t a = packed[col * 32 + j], b = packed[col * 32 + 16 + j];
    const uint32_t hi = v < 16 ? (a & 15u) : (a >> 4);
    const uint32_t lo = v < 16 ? (b & 15u) : (b >> 4);
    return (hi << 4) | lo;
}

// lane v of one record: reference record [D*4 codes | 96 f32] -> device block [Dc*4 | 96 f32] (k_relayout_blocks)
__device__ __forceinline__ void load_batch_record(const uint8_t* __restrict__ rec, uint8_t* __restrict__ dst, uint32_t D, uint32_t Dc,
                                                  uint32_t v) {
    const uint32_t ncol = D / 8, G16 = Dc >> 7;
    for (uint32_t g = 0; g < G16; ++g) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t c = 0; c < 16; ++c) {
            const uint32_t col = g * 16 + c;
            if (col < ncol) w[c >> 2] |= load_fastscan_byte(rec, col, v) << (8 * (c & 3));
        }
        *reinterpret_cast<uint4*>(dst + (size_t)g * 512 + v * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (Dc & 64u) {
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
            const uint32_t col = G16 * 16 + c;
            if (col < ncol) w[c >> 2] |= load_fastscan_byte(rec, col, v) << (8 * (c & 3));
        }
        *reinterpret_cast<uint2*>(dst + (size_t)G16 * 512 + v * 8) = make_uint2(w[0], w[1]);
    }
    const uint8_t* fs = rec + (size_t)D * 4;
    uint32_t* fd = reinterpret_cast<uint32_t*>(dst + (size_t)Dc * 4);
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) fd[r * 32 + v] = ld32(fs + (r * 32 + v) * 4);
}

// lane l of 16 of one slot: packed ex code (or none: a pad slot) -> the slot's lane-major units (k_relayout_ex)
__device__ __forceinline__ void load_ex_code(const uint8_t* __restrict__ src, bool valid, uint8_t* __restrict__ slot_dst, uint32_t D,
                                             uint32_t ex_bits, uint32_t l) {
    const uint32_t w4 = ex_w4(D, ex_bits), cpu = ex_cpu(ex_bits);
    uint4* dst = reinterpret_cast<uint4*>(slot_dst) + l;
    uint32_t t = 0;
    for (uint32_t unit = 0; unit < w4; ++unit) {
        uint32_t u[5] = {0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < cpu && t < D / 16; ++k, ++t) {
            uint32_t code = 0;
            if (valid) {
                if (ex_bits == 2) {
                    code = ((uint32_t)src[t * 4 + (l & 3u)] >> (2 * (l >> 2))) & 3u;
                } else {
                    const uint32_t lo = src[t * 12 + (l & 7u)], hi = src[t * 12 + 8 + (l & 3u)];
                    code = ((lo >> (l < 8 ? 0 : 4)) & 15u) | (((hi >> (2 * (l >> 2))) & 3u) << 4);
                }
            }
            const uint32_t bit = k * ex_bits, idx = bit >> 5, sh = bit & 31u;
            u[idx] |= code << sh;
            if (sh + ex_bits > 32) u[idx + 1] |= code >> (32 - sh);
        }
        dst[unit * 16] = make_uint4(u[0], u[1], u[2], u[3]);
    }
}

__device__ __forceinline__ void load_check_prefix(const uint8_t* __restrict__ p, uint64_t exb, uint64_t file_pos,
                                                  unsigned long long* __restrict__ bad) {
    uint64_t el = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) el |= (uint64_t)p[i] << (8 * i);
    if (el != exb) atomicMin(bad, (unsigned long long)file_pos);
}

__global__ __launch_bounds__(256) void k_load_span(LoadSpanParams P) {
    const uint32_t w = blockIdx.x, tid = threadIdx.x;
    uint32_t lo = 0, hi = P.n_pieces; // the largest p with wg0[p] <= w (pieces without workgroups share the next one's wg0)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (P.pieces[mid].wg0 <= w) lo = mid; else hi = mid;
    }
    const LoadPiece pc = P.pieces[lo];
    const uint32_t t = w - pc.wg0, slots = pc.count + pc.fill;
    const uint8_t* src = P.span + pc.off;
    switch (pc.kind) {
        case rbq_host::kLpCentroid: {
            const uint32_t i = t * 256 + tid;
            if (i < pc.count) P.centroids[pc.first + i] = ld32(src + (size_t)i * 4);
            break;
        }
        case rbq_host::kLpIds: {
            const uint32_t i = t * 256 + tid;
            if (i < slots)
                P.ids[pc.first + i] = i < pc.count ? (uint64_t)ld32(src + (size_t)i * 8) | ((uint64_t)ld32(src + (size_t)i * 8 + 4) << 32) : ~0ull;
            break;
        }
        case rbq_host::kLpFadd: case rbq_host::kLpFres: case rbq_host::kLpDelta: case rbq_host::kLpVl: {
            uint32_t* dst = pc.kind == rbq_host::kLpFadd ? P.fadd_ex : pc.kind == rbq_host::kLpFres ? P.fres_ex
                          : pc.kind == rbq_host::kLpDelta ? P.delta : P.vl;
            const uint32_t i = t * 256 + tid;
            if (i < slots) dst[pc.first + i] = i < pc.count ? ld32(src + (size_t)i * 4) : 0u;
            break;
        }
        case rbq_host::kLpBatch: {
            const uint32_t r = t * 8 + (tid >> 5);
            if (r < pc.count)
                load_batch_record(src + (size_t)r * ((size_t)P.D * 4 + 384), P.blocks + (size_t)(pc.first + r) * ((size_t)P.Dc * 4 + 384), P.D,
                                  P.Dc, tid & 31u);
            break;
        }
        case rbq_host::kLpEx: {
            const uint64_t rec = 8 + P.exb;
            if (P.scatter && P.ex_bits) {
                const uint32_t s = t * 16 + (tid >> 4), l = tid & 15u;
                if (s >= slots) break;
                const bool valid = s < pc.count;
                const uint8_t* e = src + (size_t)s * rec;
                if (valid && l == 0) load_check_prefix(e, P.exb, P.span_off + pc.off + (uint64_t)s * rec, P.bad_prefix);
                load_ex_code(e + 8, valid, P.ex + (size_t)(pc.first + s) * ex_bytes_dev(P.D, P.ex_bits), P.D, P.ex_bits, l);
            } else {
                const uint32_t i = t * 256 + tid;
                if (i < pc.count) load_check_prefix(src + (size_t)i * rec, P.exb, P.span_off + pc.off + (uint64_t)i * rec, P.bad_prefix);
            }
            break;
        }
        default: break;
    }
}

__global__ __launch_bounds__(256) void k_load_block_nv(const uint32_t* __restrict__ list_gb0, const uint32_t* __restrict__ list_n,
                                                       uint32_t n_lists, uint32_t* __restrict__ block_nv) {
    const uint32_t c = blockIdx.x;
    if (c >= n_lists) return;
    const uint32_t n = list_n[c], nb = (n + 31u) / 32u, gb0 = list_gb0[c];
    for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) block_nv[gb0 + b] = b + 1 == nb ? n - b * 32u : 32u;
}

} // namespace

hipError_t launch_load_span(const LoadSpanParams& P, uint64_t n_workgroups, hipStream_t s) {
    if (!n_workgroups) return hipSuccess;
    if (n_workgroups > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_load_span, dim3((uint32_t)n_workgroups), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_load_block_nv(const uint32_t* list_gb0, const uint32_t* list_n, uint32_t n_lists, uint32_t* block_nv, hipStream_t s) {
    if (!n_lists) return hipSuccess;
    hipLaunchKernelGGL(k_load_block_nv, dim3(n_lists), dim3(256), 0, s, list_gb0, list_n, n_lists, block_nv);
    return hipGetLastError();
}

} // namespace rbq
