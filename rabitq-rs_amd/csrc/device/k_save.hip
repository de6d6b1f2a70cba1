// k_save.hip — translation unit of the RBQ1 writer's kernels (rbq_index_save_rbq1, include/rbq_persist.h).  gfx950 only.
//
//   k_save_fill      the cluster section of the stream (save_to_writer, src/ivf.rs:1310-1474), one 32-bit word per thread:
//                    the inverse of k_relayout_blocks (lane-major granules -> pack_codes' FastScan record), of
//                    k_relayout_ex (lane-major units -> pack_ex2 / pack_ex6, each with its u64 length prefix) and of
//                    k_spread (slot order -> dense list order, pad slots dropped)
//   k_crc_segments   CRC-32/IEEE of fixed-size segments of a byte range, slice-by-4 tables in LDS
//   k_crc_reduce     one workgroup folds the segment CRCs with zlib's crc32_combine (rbq_host_logic.hpp)
// (the code decoders dev_code_byte / dev_ex_code live in codes.hpp, shared with k_fetch.hip)
//
// Every section of the cluster part is a multiple of 4 bytes long (D % 16 == 0), so the section starts at a word
// boundary of the stream and a thread owns exactly one word; u64 fields are written as two words.  A word finds its
// cluster by binary search over the clusters' word offsets, so a chunk may begin and end anywhere, inside a cluster too.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "kernels.hpp"
#include "codes.hpp"

namespace rbq {

namespace {

__device__ __forceinline__ uint32_t f32_bits(const float* __restrict__ a, size_t i) { return __float_as_uint(a[i]); }

__global__ __launch_bounds__(256) void k_save_fill(SaveParams P, uint64_t w0, uint64_t nw, uint32_t* __restrict__ out) {
    const uint32_t D = P.D, ex_bits = P.ex_bits, exw = P.ex_words, G16 = P.Dc >> 7;
    const size_t dev_stride = (size_t)P.Dc * 4 + 384;
    const uint64_t rec_w = (uint64_t)D + 96; // words of one reference record
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t w = w0 + i;
        uint32_t lo = 0, hi = P.n_lists; // largest c with woff[c] <= w (every cluster is at least D + 4 words long)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.woff[mid] <= w) lo = mid; else hi = mid;
        }
        const uint32_t c = lo;
        const uint64_t n = P.list_n[c], nb = (n + 31) / 32, s0 = (uint64_t)P.list_gb0[c] * 32;
        uint64_t q = w - P.woff[c];
        uint32_t word = 0;
        if (q < D) { out[i] = f32_bits(P.centroids, (size_t)c * D + q); continue; }
        q -= D;
        if (q < 2) { out[i] = q == 0 ? (uint32_t)n : (uint32_t)(n >> 32); continue; }
        q -= 2;
        if (q < 2 * n) {
            const uint64_t id = P.ids[s0 + (q >> 1)];
            out[i] = (q & 1) ? (uint32_t)(id >> 32) : (uint32_t)id;
            continue;
        }
        q -= 2 * n;
        if (q < 2) {
            const uint64_t blen = nb * rec_w * 4;
            out[i] = q == 0 ? (uint32_t)blen : (uint32_t)(blen >> 32);
            continue;
        }
        q -= 2;
        if (q < nb * rec_w) {
            const uint64_t b = q / rec_w;
            const uint32_t r = (uint32_t)(q - b * rec_w);
            const uint8_t* blk = P.blocks + (size_t)(s0 / 32 + b) * dev_stride;
            if (r < D) { // pack_codes: byte p = 32 col + j' of the record; j = j' & 15, the high (j' < 16) or low nibbles of
                         // vectors KPERM0[j] and KPERM0[j] + 16, KPERM0[j] = (j >> 1) + 8 (j & 1)
                const uint32_t col = r >> 3, jb = (r & 7u) * 4;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t jj = jb + k, j = jj & 15u, u = (j >> 1) + 8u * (j & 1u);
                    const uint32_t a = dev_code_byte(blk, G16, col, u), bb = dev_code_byte(blk, G16, col, u + 16);
                    const uint32_t na = jj < 16 ? a >> 4 : a & 15u, nbb = jj < 16 ? bb >> 4 : bb & 15u;
                    word |= (na | (nbb << 4)) << (8 * k);
                }
            } else {
                word = reinterpret_cast<const uint32_t*>(blk + (size_t)P.Dc * 4)[r - D]; // factor rows, all 32 lanes
            }
            out[i] = word;
            continue;
        }
        q -= nb * rec_w;
        const uint64_t per = 2 + (uint64_t)exw;
        if (q < n * per) {
            const uint64_t v = q / per;
            const uint32_t r = (uint32_t)(q - v * per);
            if (r < 2) { out[i] = r == 0 ? exw * 4 : 0u; continue; }
            const uint8_t* exs = P.ex + (s0 + v) * P.exd;
            const uint32_t e = r - 2;
            if (ex_bits == 2) { // pack_ex2: byte m of group t, bits 2g = code 16t + 4g + m
                const uint32_t t = e;
#pragma unroll
                for (uint32_t m = 0; m < 4; ++m)
#pragma unroll
                    for (uint32_t g = 0; g < 4; ++g) word |= dev_ex_code(exs, P.cpu, 2, 16 * t + 4 * g + m) << (8 * m + 2 * g);
            } else {            // pack_ex6: 12 bytes per group t; bytes 0-7 low nibbles of dims m and m + 8, 8-11 the top two bits
                const uint32_t t = e / 3, kk = e - t * 3;
                if (kk < 2) {
#pragma unroll
                    for (uint32_t m = 0; m < 4; ++m) {
                        const uint32_t j = kk * 4 + m;
                        word |= ((dev_ex_code(exs, P.cpu, 6, 16 * t + j) & 15u) | ((dev_ex_code(exs, P.cpu, 6, 16 * t + j + 8) & 15u) << 4)) << (8 * m);
                    }
                } else {
#pragma unroll
                    for (uint32_t m = 0; m < 4; ++m)
#pragma unroll
                        for (uint32_t g = 0; g < 4; ++g) word |= ((dev_ex_code(exs, P.cpu, 6, 16 * t + 4 * g + m) >> 4) & 3u) << (8 * m + 2 * g);
                }
            }
            out[i] = word;
            continue;
        }
        q -= n * per;
        const uint32_t arr = (uint32_t)(q / n); // 0 f_add_ex, 1 f_rescale_ex, 2 delta, 3 vl
        const uint64_t v = q - (uint64_t)arr * n;
        if (arr < 2) word = ex_bits ? f32_bits(arr == 0 ? P.fadd_ex : P.fres_ex, s0 + v) : 0u; // 1-bit: the trainer's 0.0
        else word = f32_bits(arr == 2 ? P.delta : P.vl, s0 + v);
        out[i] = word;
    }
}

// CRC-32/IEEE tables: t[0] the byte table, t[k][b] = t[k-1][b] >> 8 ^ t[0][t[k-1][b] & 0xff] (slice-by-4)
__device__ __forceinline__ void crc_tables(uint32_t (*t)[256]) {
    for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x) {
        uint32_t c = b;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        t[0][b] = c;
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x) {
        uint32_t c = t[0][b];
        for (int k = 1; k < 4; ++k) { c = (c >> 8) ^ t[0][c & 0xff]; t[k][b] = c; }
    }
    __syncthreads();
}

// segment s = bytes [s * seg, min(n, (s + 1) * seg)) of p (any alignment): its own CRC-32 (init ~0, final ~)
__global__ __launch_bounds__(256) void k_crc_segments(const uint8_t* __restrict__ p, uint64_t n, uint32_t seg, uint64_t nseg,
                                                      uint32_t* __restrict__ seg_crc) {
    __shared__ uint32_t t[4][256];
    crc_tables(t);
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const uint8_t* a = p + s * seg;
    const uint8_t* e = p + (s * seg + seg < n ? s * seg + seg : n);
    uint32_t c = ~0u;
    while (a < e && ((uintptr_t)a & 15u)) c = t[0][(c ^ *a++) & 0xff] ^ (c >> 8);
    auto word = [&](uint32_t x) {
        x ^= c;
        c = t[3][x & 0xff] ^ t[2][(x >> 8) & 0xff] ^ t[1][(x >> 16) & 0xff] ^ t[0][x >> 24];
    };
    while (e - a >= 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(a);
        word(v.x); word(v.y); word(v.z); word(v.w);
        a += 16;
    }
    while (a < e) c = t[0][(c ^ *a++) & 0xff] ^ (c >> 8);
    seg_crc[s] = ~c;
}

// GF(2) arithmetic of crc32_combine (rbq_host_logic.hpp: crc32_multmodp / crc32_x8nmodp)
__device__ uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
__device__ uint32_t x8nmodp(uint64_t n) {
    uint32_t p = 1u << 31, sq = 1u << 23;
    while (n) {
        if (n & 1) p = multmodp(sq, p);
        sq = multmodp(sq, sq);
        n >>= 1;
    }
    return p;
}

// one workgroup: crc32(p[0, n)) from the nseg segment CRCs (segments of `seg` bytes, the last one shorter)
__global__ __launch_bounds__(256) void k_crc_reduce(const uint32_t* __restrict__ seg_crc, uint64_t nseg, uint32_t seg, uint64_t n,
                                                    uint32_t* __restrict__ out) {
    __shared__ uint32_t s_crc[256];
    __shared__ uint64_t s_len[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (nseg + 255) / 256, a = tid * per < nseg ? tid * per : nseg, e = a + per < nseg ? a + per : nseg;
    const uint32_t xfull = x8nmodp(seg);
    uint32_t crc = 0;
    uint64_t len = 0;
    for (uint64_t s = a; s < e; ++s) {
        const uint64_t l = s + 1 == nseg ? n - s * (uint64_t)seg : seg;
        crc = len == 0 ? seg_crc[s] : multmodp(l == seg ? xfull : x8nmodp(l), crc) ^ seg_crc[s];
        len += l;
    }
    s_crc[tid] = crc;
    s_len[tid] = len;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) { // (left, right) -> left || right; empty spans fold to nothing
        uint32_t nc = 0;
        uint64_t nl = 0;
        const bool act = (tid & (2 * d - 1)) == 0 && tid + d < 256;
        if (act) {
            const uint32_t lc = s_crc[tid], rc = s_crc[tid + d];
            const uint64_t ll = s_len[tid], rl = s_len[tid + d];
            nc = rl == 0 ? lc : ll == 0 ? rc : multmodp(x8nmodp(rl), lc) ^ rc;
            nl = ll + rl;
        }
        __syncthreads();
        if (act) { s_crc[tid] = nc; s_len[tid] = nl; }
        __syncthreads();
    }
    if (tid == 0) *out = s_crc[0];
}

} // namespace

hipError_t launch_save_fill(const SaveParams& P, uint64_t w0, uint64_t nw, uint32_t* out, hipStream_t s) {
    if (!nw) return hipSuccess;
    const uint64_t blocks = (nw + 255) / 256;
    hipLaunchKernelGGL(k_save_fill, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, P, w0, nw, out);
    return hipGetLastError();
}

uint64_t crc_scratch_words(uint64_t n) { return (n + kCrcSegment - 1) / kCrcSegment; }

hipError_t launch_crc32(const uint8_t* p, uint64_t n, uint32_t* seg_scratch, uint32_t* out, hipStream_t s) {
    if (!n) return hipMemsetAsync(out, 0, 4, s);
    const uint64_t nseg = crc_scratch_words(n);
    hipLaunchKernelGGL(k_crc_segments, dim3((uint32_t)((nseg + 255) / 256)), dim3(256), 0, s, p, n, kCrcSegment, nseg, seg_scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_crc_reduce, dim3(1), dim3(256), 0, s, (const uint32_t*)seg_scratch, nseg, kCrcSegment, n, out);
    return hipGetLastError();
}

} // namespace rbq
