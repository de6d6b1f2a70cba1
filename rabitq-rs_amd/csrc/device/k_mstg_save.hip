// k_mstg_save.hip — translation unit of the `.mstg` writer's and loader's kernels (include/rbq_mstg_persist.h; the format and
// its lengths: csrc/host/rbq_mstg_file.hpp).  gfx950 only.
//
//   k_mstg_save_fill     a byte range of the posting-list section of the stream from the device layout: the list headers
//                        (length prefix, cluster_id, centroid, size, RabitqConfig, vectors.len()) and one bincode record per
//                        vector — id, code = ex_code + (bit << ex_bits) as u16, the sign bits out of the granules
//                        (binary_code_packed, MSB first), the ex units re-packed as pack_ex2 / pack_ex6 (the cpp-compat layout of
//                        src/simd.rs:2478-2541, 2601-2695 is the one RBQ1 stores, so k_save_fill's formulas serve), ex_bits, dim
//                        and the eight factors (f_add, f_rescale, f_error from the block's factor rows, the rest from the slot
//                        arrays)
//   k_mstg_load_scatter  the inverse: one workgroup per 32-vector block reads the block's records out of an uploaded span of the
//                        stream, writes granules, ex units, factor rows, ids and the slot arrays (pad slots as the encoder leaves
//                        them: codes and factors 0, id ~0) and validates every record's inner fields into an error word
//
// A record is 73 + 2 D + D / 8 + E bytes long — odd — so records begin at every alignment and nothing in the section is
// word-aligned.  The fill therefore works on the OUTPUT's words: thread i owns word i of the staging buffer, which holds
// section bytes b0 + 4 i .. b0 + 4 i + 3 whatever b0 is, finds the list by binary search and the record by one division, and
// forms its four bytes; stores are one coalesced dword per lane, and a chunk may begin and end anywhere, inside a length field
// too.  When all four bytes lie in one record (all but two words per record) the division is shared.
// The CRC of the bytes is k_save.hip's (launch_crc32).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "kernels.hpp"
#include "codes.hpp"
#include "../host/rbq_mstg_file.hpp"

namespace rbq {

namespace {

using rbq_host::kMstgBadBinLen;
using rbq_host::kMstgBadCode;
using rbq_host::kMstgBadCodeLen;
using rbq_host::kMstgBadDim;
using rbq_host::kMstgBadExBits;
using rbq_host::kMstgBadExLen;
using rbq_host::kMstgBadOneBit;

__device__ __forceinline__ uint32_t byte_of(uint64_t v, uint32_t k) { return (uint32_t)(v >> (8u * k)) & 0xffu; }

// byte e of pack_ex2 / pack_ex6 of a slot's ex codes (k_save_fill's formulas, a byte at a time)
__device__ __forceinline__ uint32_t ex_packed_byte(const uint8_t* __restrict__ exs, uint32_t cpu, uint32_t ex_bits, uint32_t e) {
    uint32_t b = 0;
    if (ex_bits == 2) { // byte m of group t: bits 2g = code 16t + 4g + m
        const uint32_t t = e >> 2, m = e & 3u;
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) b |= dev_ex_code(exs, cpu, 2, 16 * t + 4 * g + m) << (2 * g);
    } else if (ex_bits == 6) { // 12 bytes per group t: 0-7 the low nibbles of dims m and m + 8, 8-11 the top two bits
        const uint32_t t = e / 12, kk = e - t * 12;
        if (kk < 8) {
            b = (dev_ex_code(exs, cpu, 6, 16 * t + kk) & 15u) | ((dev_ex_code(exs, cpu, 6, 16 * t + kk + 8) & 15u) << 4);
        } else {
            const uint32_t m = kk - 8;
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g) b |= ((dev_ex_code(exs, cpu, 6, 16 * t + 4 * g + m) >> 4) & 3u) << (2 * g);
        }
    }
    return b; // ex_bits == 0: D / 16 * 2 zero bytes
}

// byte r of the record of `slot`
__device__ uint32_t rec_byte(const MstgSaveParams& P, uint64_t slot, uint32_t r) {
    const uint32_t D = P.D, ex_bits = P.ex_bits, G16 = P.Dc >> 7, v = (uint32_t)slot & 31u;
    const uint8_t* blk = P.blocks + (slot >> 5) * ((size_t)P.Dc * 4 + 384);
    const uint8_t* exs = P.ex + slot * P.exd;
    if (r < 8) return byte_of(P.ids[slot], r);
    r -= 8;
    if (r < 8) return byte_of(D, r);
    r -= 8;
    if (r < 2 * D) { // code: u16 per dimension
        const uint32_t d = r >> 1;
        const uint32_t bit = (dev_code_byte(blk, G16, d >> 3, v) >> (7u - (d & 7u))) & 1u;
        const uint32_t code = (ex_bits ? dev_ex_code(exs, P.cpu, ex_bits, d) : 0u) + (bit << ex_bits);
        return (code >> (8u * (r & 1u))) & 0xffu;
    }
    r -= 2 * D;
    if (r < 8) return byte_of(D / 8, r);
    r -= 8;
    if (r < D / 8) return dev_code_byte(blk, G16, r, v);
    r -= D / 8;
    if (r < 8) return byte_of(P.E, r);
    r -= 8;
    if (r < P.E) return ex_packed_byte(exs, P.cpu, ex_bits, r);
    r -= P.E;
    if (r == 0) return ex_bits;
    r -= 1;
    if (r < 8) return byte_of(D, r);
    r -= 8;
    const float* fac = reinterpret_cast<const float*>(blk + (size_t)P.Dc * 4);
    const uint32_t f = r >> 2;
    uint32_t w;
    switch (f) { // delta, vl, f_add, f_rescale, f_error, residual_norm, f_add_ex, f_rescale_ex
        case 0: w = __float_as_uint(P.delta[slot]); break;
        case 1: w = __float_as_uint(P.vl[slot]); break;
        case 2: w = __float_as_uint(fac[v]); break;
        case 3: w = __float_as_uint(fac[32 + v]); break;
        case 4: w = __float_as_uint(fac[64 + v]); break;
        case 5: w = __float_as_uint(P.rnorm[slot]); break;
        case 6: w = ex_bits ? __float_as_uint(P.fadd_ex[slot]) : 0u; break; // 1-bit: the quantizer's 0.0
        default: w = ex_bits ? __float_as_uint(P.fres_ex[slot]) : 0u; break;
    }
    return (w >> (8u * (r & 3u))) & 0xffu;
}

// byte q (counted from the list's u64 length prefix, q < 8 + hdr) of list c's prefix and header
__device__ uint32_t head_byte(const MstgSaveParams& P, uint32_t c, uint32_t n, uint32_t tag, uint64_t body, uint32_t q) {
    const uint32_t D = P.D;
    if (q < 8) return byte_of(body, q);
    q -= 8;
    if (q < 4) return byte_of(c, q);
    q -= 4;
    if (q < 8) return byte_of(D, q);
    q -= 8;
    if (q < 4 * D) return byte_of(__float_as_uint(P.centroids[(size_t)c * D + (q >> 2)]), q & 3u);
    q -= 4 * D;
    if (q < 4) return byte_of(n, q);
    q -= 4;
    if (q < 8) return byte_of(n ? P.ex_bits + 1u : 7u, q); // an empty list keeps RabitqConfig::default()
    q -= 8;
    if (q == 0) return tag;
    q -= 1;
    if (tag) {
        if (q < 4) return byte_of(P.t_bits, q);
        q -= 4;
    }
    return byte_of(n, q);
}

__global__ __launch_bounds__(256) void k_mstg_save_fill(MstgSaveParams P, uint64_t b0, uint64_t nb, uint32_t* __restrict__ out) {
    const uint64_t nw = (nb + 3) / 4, R = P.R;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t pos = b0 + 4 * i;
        const uint32_t live = nb - 4 * i < 4 ? (uint32_t)(nb - 4 * i) : 4u; // bytes of this word inside the chunk
        uint32_t lo = 0, hi = P.n_lists; // largest c with loff[c] <= pos
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.loff[mid] <= pos) lo = mid; else hi = mid;
        }
        uint32_t c = lo, word = 0, j = 0;
        while (j < live) { // (a word leaves a list at most once: every list is longer than 4 bytes)
            const uint64_t base = P.loff[c], q = pos - base, len = P.loff[c + 1] - base;
            const uint32_t n = P.list_n[c], tag = n ? P.has_t : 0u;
            const uint64_t hdr = 8 + 33 + 4ull * P.D + (tag ? 4u : 0u);
            if (q >= len) { ++c; continue; }
            if (q < hdr) {
                word |= head_byte(P, c, n, tag, len - 8, (uint32_t)q) << (8 * j);
                ++j; ++pos;
                continue;
            }
            const uint64_t v = (q - hdr) / R;
            uint32_t r = (uint32_t)((q - hdr) - v * R);
            const uint64_t slot = (uint64_t)P.list_gb0[c] * 32 + v;
            for (; j < live && r < R; ++j, ++r, ++pos) word |= rec_byte(P, slot, r) << (8 * j);
        }
        out[i] = word;
    }
}

// little-endian u64 at any alignment
__device__ __forceinline__ uint64_t ld64(const uint8_t* __restrict__ p) {
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
    return v;
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* __restrict__ p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// the ex code of dimension i in a record's ex_code_packed (k_relayout_ex's formulas)
__device__ __forceinline__ uint32_t packed_ex_code(const uint8_t* __restrict__ ex, uint32_t ex_bits, uint32_t i) {
    const uint32_t t = i >> 4, l = i & 15u;
    if (ex_bits == 2) return ((uint32_t)ex[t * 4 + (l & 3u)] >> (2 * (l >> 2))) & 3u;
    if (ex_bits == 6) {
        const uint32_t lo = ex[t * 12 + (l & 7u)], hi = ex[t * 12 + 8 + (l & 3u)];
        return ((lo >> (l < 8 ? 0 : 4)) & 15u) | (((hi >> (2 * (l >> 2))) & 3u) << 4);
    }
    return 0u;
}

__global__ __launch_bounds__(256) void k_mstg_load_scatter(MstgLoadParams P) {
    const uint32_t b = P.gb_first + blockIdx.x, tid = threadIdx.x;
    const uint32_t D = P.D, Dc = P.Dc, ex_bits = P.ex_bits, R = P.R, E = P.E, G16 = Dc >> 7, ncol = D / 8;
    const uint32_t nv = P.block_nv[b];
    const uint8_t* src = P.span + (P.boff[b] - P.span_off); // nv records of R bytes
    const uint32_t o_bin = 16 + 2 * D, o_ex = o_bin + 8 + ncol, o_tail = o_ex + 8 + E;
    uint8_t* blk = P.blocks + (size_t)b * ((size_t)Dc * 4 + 384);
    const size_t exd = ex_bytes_dev(D, ex_bits);
    uint32_t flags = 0;

    // ids, inner lengths, factors: lane v of the first half-wave
    if (tid < 32) {
        const uint32_t v = tid;
        const size_t slot = (size_t)b * 32 + v;
        const bool real = v < nv;
        const uint8_t* r = src + (size_t)v * R;
        uint32_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t id = ~0ull;
        if (real) {
            id = ld64(r);
            if (ld64(r + 8) != D) flags |= kMstgBadCodeLen;
            if (ld64(r + o_bin) != ncol) flags |= kMstgBadBinLen;
            if (ld64(r + o_ex) != E) flags |= kMstgBadExLen;
            if (r[o_tail] != ex_bits) flags |= kMstgBadExBits;
            if (ld64(r + o_tail + 1) != D) flags |= kMstgBadDim;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) f[k] = ld32(r + o_tail + 9 + 4 * k);
            if (ex_bits == 0 && (f[6] | f[7])) flags |= kMstgBadOneBit;
        }
        uint32_t* fac = reinterpret_cast<uint32_t*>(blk + (size_t)Dc * 4);
        P.ids[slot] = id;
        reinterpret_cast<uint32_t*>(P.delta)[slot] = f[0];
        reinterpret_cast<uint32_t*>(P.vl)[slot] = f[1];
        fac[v] = f[2]; fac[32 + v] = f[3]; fac[64 + v] = f[4];
        reinterpret_cast<uint32_t*>(P.rnorm)[slot] = f[5];
        if (ex_bits) {
            reinterpret_cast<uint32_t*>(P.fadd_ex)[slot] = f[6];
            reinterpret_cast<uint32_t*>(P.fres_ex)[slot] = f[7];
        }
    }

    // granules: (vector, granule) per thread; 16 code bytes of 128 dims, the half granule of Dc % 128 == 64 last
    const uint32_t ngran = G16 + ((Dc & 64u) ? 1u : 0u);
    for (uint32_t task = tid; task < 32 * ngran; task += 256) {
        const uint32_t v = task & 31u, g = task >> 5;
        const uint8_t* bin = src + (size_t)v * R + o_bin + 8;
        uint32_t w[4] = {0, 0, 0, 0};
        const uint32_t nbytes = g < G16 ? 16u : 8u;
#pragma unroll
        for (uint32_t cix = 0; cix < 16; ++cix) {
            const uint32_t col = g * 16 + cix;
            if (cix < nbytes && v < nv && col < ncol) w[cix >> 2] |= (uint32_t)bin[col] << (8 * (cix & 3u));
        }
        if (g < G16) *reinterpret_cast<uint4*>(blk + (size_t)g * 512 + v * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        else *reinterpret_cast<uint2*>(blk + (size_t)G16 * 512 + v * 8) = make_uint2(w[0], w[1]);
    }

    // ex units: 16 lanes per vector, lane l owns dims 16t + l (k_relayout_ex)
    if (ex_bits) {
        const uint32_t w4 = ex_w4(D, ex_bits), cpu = ex_cpu(ex_bits);
        for (uint32_t task = tid; task < 512; task += 256) {
            const uint32_t v = task >> 4, l = task & 15u;
            const uint8_t* ex = src + (size_t)v * R + o_ex + 8;
            uint4* dst = reinterpret_cast<uint4*>(P.ex + ((size_t)b * 32 + v) * exd) + l;
            uint32_t t = 0;
            for (uint32_t unit = 0; unit < w4; ++unit) {
                uint32_t u[5] = {0, 0, 0, 0, 0};
                for (uint32_t k = 0; k < cpu && t < D / 16; ++k, ++t) {
                    const uint32_t code = v < nv ? packed_ex_code(ex, ex_bits, 16 * t + l) : 0u;
                    const uint32_t bit = k * ex_bits, idx = bit >> 5, sh = bit & 31u;
                    u[idx] |= code << sh;
                    if (sh + ex_bits > 32) u[idx + 1] |= code >> (32 - sh);
                }
                dst[unit * 16] = make_uint4(u[0], u[1], u[2], u[3]);
            }
        }
    }

    // code[i] == ex_code[i] + (bit[i] << ex_bits); a 1-bit record's ex bytes are zero
    for (uint32_t task = tid; task < nv * D; task += 256) {
        const uint32_t v = task / D, i = task - v * D;
        const uint8_t* r = src + (size_t)v * R;
        const uint32_t have = (uint32_t)r[16 + 2 * i] | ((uint32_t)r[17 + 2 * i] << 8);
        const uint32_t bit = ((uint32_t)r[o_bin + 8 + (i >> 3)] >> (7u - (i & 7u))) & 1u;
        if (have != packed_ex_code(r + o_ex + 8, ex_bits, i) + (bit << ex_bits)) flags |= kMstgBadCode;
    }
    if (ex_bits == 0)
        for (uint32_t task = tid; task < nv * E; task += 256) {
            const uint32_t v = task / E, e = task - v * E;
            if (src[(size_t)v * R + o_ex + 8 + e]) flags |= kMstgBadOneBit;
        }
    if (flags) atomicOr(P.err, flags);
}

} // namespace

hipError_t launch_mstg_save_fill(const MstgSaveParams& P, uint64_t b0, uint64_t nb, uint32_t* out, hipStream_t s) {
    if (!nb) return hipSuccess;
    const uint64_t blocks = ((nb + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(k_mstg_save_fill, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, P, b0, nb, out);
    return hipGetLastError();
}

hipError_t launch_mstg_load_scatter(const MstgLoadParams& P, hipStream_t s) {
    if (!P.nb) return hipSuccess;
    hipLaunchKernelGGL(k_mstg_load_scatter, dim3(P.nb), dim3(256), 0, s, P);
    return hipGetLastError();
}

} // namespace rbq
