// rerank_score.hpp — the canonical exact scorer of a raw row on eight lanes (gfx950, wave64): the bits of canon_l2 / canon_dot
// (kernels.hpp; l2_distance_sqr / dot of src/math.rs).  One copy, shared by k_rerank_pool (k_rerank_pool.hip, DESIGN.md sections 27
// and 28) and the exact range scan (k_range<..., XR, XIP>, range.hpp).
//
// Eight lanes serve one candidate, lane j of the eight owns accumulator j.  The raw row is NOT read the way the accumulators consume
// it (lane j element 8 m + j: 4 bytes per lane, 32 bytes per candidate and load): each lane loads 16 bytes, the eight lanes one
// contiguous 128-byte span of the row, kRpSpans spans per step and the next step's already in flight; lane permutes then hand every
// lane its elements, which it adds to its chain in the order of the serial loop.  The sum -0.0 + acc[0] + ... + acc[7] and the scalar
// tail dim & ~7 .. dim follow in their order on every lane of the eight.  d * d and + stay two operations: every unit that includes
// this header is compiled with contraction off (#pragma clang fp contract(off) in front of the include, and -ffp-contract=off).
// Every lane of the wave must call the scorers (they exchange data with __shfl / DPP inside each group of eight).
#pragma once
#include "kernels.hpp"

namespace rbq {

constexpr uint32_t kRpSpans = 4; // 128-byte spans of a row per candidate and step (twice that in flight)

// component c of (x, y, z, w) as two levels of selects (no branch: every operand is already in a register)
__device__ __forceinline__ float rp_pick(float x, float y, float z, float w, uint32_t c) {
    const bool odd = (c & 1u) != 0u, high = (c & 2u) != 0u;
    const float lo = odd ? y : x, hi = odd ? w : z;
    return high ? hi : lo;
}
// 16 bytes at a 4-byte aligned address, one load
__device__ __forceinline__ float4 rp_load16(const float* p) {
    struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };
    const F4 v = *reinterpret_cast<const F4*>(p);
    return make_float4(v.x, v.y, v.z, v.w);
}

// The canonical score of one row of f32 elements on the eight lanes of a group (j: the lane's index in its group, base: the wave lane
// of the group's first).  Round t of a span's four permutes: lane j receives chunk m = (t + j) & 3 from lane 2 m + (j >> 2), which
// published component ((lane >> 1) - t) & 3 — so every source lane serves four different readers one component each — and the lane
// adds them to its chain in the order m = 0 .. 3.  Rows start 4 dim bytes apart, so a span is 4-byte aligned only: the 16-byte loads
// are issued as such (global loads of this target need dword alignment, not more).  Every lane loads, without a branch: a span that
// does not lie wholly in the row's main part is replaced by the row's first 16 bytes (Dmain >= 8 there; its chunks are never
// accumulated), so nothing outside the row is read.
template <bool IP>
__device__ __forceinline__ float rp_score32(const float* row, const float* sq, uint32_t dim, uint32_t j, uint32_t base) {
    const uint32_t Dmain = dim & ~7u;
    const uint32_t jq = j & 3u, jh = j >> 2;
    float acc = 0.0f;
    auto load_spans = [&](float4* v, uint32_t e0) {
#pragma unroll
        for (uint32_t s = 0; s < kRpSpans; ++s) {
            const uint32_t e = e0 + 32u * s + 4u * j;
            v[s] = rp_load16(row + (e + 4u <= Dmain ? e : 0u));
        }
    };
    float4 v[kRpSpans], nx[kRpSpans];
    if (Dmain) load_spans(v, 0u);
    for (uint32_t e0 = 0; e0 < Dmain; e0 += 32u * kRpSpans) {
        load_spans(nx, e0 + 32u * kRpSpans); // the next spans travel while these are consumed
#pragma unroll
        for (uint32_t s = 0; s < kRpSpans; ++s) {
            float w[4];
#pragma unroll
            for (uint32_t t = 0; t < 4u; ++t) {
                const float mine = rp_pick(v[s].x, v[s].y, v[s].z, v[s].w, ((j >> 1) - t) & 3u);
                const uint32_t m = (t + jq) & 3u;
                w[t] = __shfl(mine, (int)(base | (2u * m + jh)));
            }
#pragma unroll
            for (uint32_t m = 0; m < 4u; ++m) {
                const uint32_t c0 = e0 + 32u * s + 8u * m; // chunk of eight elements (wave-uniform)
                if (c0 < Dmain) {
                    const float b = rp_pick(w[0], w[1], w[2], w[3], (m - jq) & 3u);
                    const float a = sq[c0 + j];
                    float p;
                    if (IP) {
                        p = a * b;
                    } else {
                        const float d = a - b;
                        p = d * d;
                    }
                    acc = acc + p;
                }
            }
        }
#pragma unroll
        for (uint32_t s = 0; s < kRpSpans; ++s) v[s] = nx[s];
    }
    float sum = 0.0f;
    if (Dmain) {
        sum = -0.0f;
#pragma unroll
        for (uint32_t l = 0; l < 8u; ++l) sum = sum + __shfl(acc, (int)(base | l));
    }
    for (uint32_t i = Dmain; i < dim; ++i) {
        const float a = sq[i], b = row[i];
        float p;
        if (IP) {
            p = a * b;
        } else {
            const float d = a - b;
            p = d * d;
        }
        sum = sum + p;
    }
    return sum;
}

// ---- rows of 16-bit elements (RAW = kRawF16 / kRawBf16) --------------------------------------------------
// eight 16-bit elements at a 4-byte aligned address, one load
__device__ __forceinline__ uint4 rp_load16h(const uint16_t* p) {
    struct __attribute__((packed, aligned(4))) U4 { uint32_t x, y, z, w; };
    const U4 v = *reinterpret_cast<const U4*>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
// the two elements of a dword (the lower half is the element at the lower address), widened exactly
template <int RAW>
__device__ __forceinline__ float rp_widen_lo(uint32_t d) {
    if (RAW == kRawF16) return (float)__builtin_bit_cast(_Float16, (uint16_t)d);
    return __uint_as_float(d << 16);
}
template <int RAW>
__device__ __forceinline__ float rp_widen_hi(uint32_t d) {
    if (RAW == kRawF16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(d >> 16));
    return __uint_as_float(d & 0xffff0000u);
}
template <int RAW>
__device__ __forceinline__ float rp_widen(uint16_t h) {
    return rp_widen_lo<RAW>(h);
}
template <bool IP>
__device__ __forceinline__ float rp_add(float acc, float a, float b) {
    float p;
    if (IP) {
        p = a * b;
    } else {
        const float d = a - b;
        p = d * d;
    }
    return acc + p;
}
// The 8 x 8 transpose of 16-bit elements over the eight lanes of a group.  In: lane l holds chunk l of a span, elements 2k, 2k+1 in
// d[k].  Out: lane j holds element j of chunk m in half m & 1 of d[m >> 1].  Three exchanges of half of the lane's data with the
// lane at distance 4, 2, 1: two dwords through ds_swizzle, two through a quad permute (DPP), then the four dwords through a quad
// permute and one v_perm_b32 each that keeps the own half and takes the partner's.  The picks are selects on lane constants
// (b0, b1, b2: the bits of the lane's index in its group; sel: the v_perm selector of its parity).  Every lane of the wave runs this.
__device__ __forceinline__ void rp_transpose8x8(uint32_t (&d)[4], bool b0, bool b1, bool b2, uint32_t sel) {
    const uint32_t s0 = b2 ? d[0] : d[2], s1 = b2 ? d[1] : d[3];
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_ds_swizzle((int)s0, 0x101f); // lane ^ 4
    const uint32_t r1 = (uint32_t)__builtin_amdgcn_ds_swizzle((int)s1, 0x101f);
    const uint32_t a00 = b2 ? r0 : d[0], a01 = b2 ? r1 : d[1], a10 = b2 ? d[2] : r0, a11 = b2 ? d[3] : r1;
    const uint32_t t0 = b1 ? a00 : a01, t1 = b1 ? a10 : a11;
    const uint32_t u0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t0, 0x4e, 0xf, 0xf, false); // quad_perm [2,3,0,1]: lane ^ 2
    const uint32_t u1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t1, 0x4e, 0xf, 0xf, false);
    const uint32_t x[4] = {b1 ? u0 : a00, b1 ? a01 : u0, b1 ? u1 : a10, b1 ? a11 : u1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x[k], 0xb1, 0xf, 0xf, false); // quad_perm [1,0,3,2]: lane ^ 1
        d[k] = __builtin_amdgcn_perm(y, x[k], sel);
    }
}
// The canonical score of one row of 16-bit elements on the eight lanes of a group (lane j: accumulator j), the same chains as the
// f32 rows take.  Span path (every row starts 4-byte aligned): a span is 64 elements, lane l loads chunk l (16 bytes), the transpose
// hands lane j element j of the chunks m = 0 .. 7, which it adds in that order.  A span that does not lie wholly inside the row's
// main part is replaced by the row's first 16 bytes and never accumulated.  by_element (rows at 2 mod 4; wave-uniform, the slow
// path): lane j loads its elements 8 m + j two bytes at a time.  Either way nothing outside the row is read.
template <bool IP, int RAW>
__device__ __forceinline__ float rp_score16(const uint16_t* row, const float* sq, uint32_t dim, uint32_t j, uint32_t base, bool by_element) {
    const uint32_t Dmain = dim & ~7u;
    float acc = 0.0f;
    if (by_element) {
        constexpr uint32_t KB = 8; // loads in flight per lane
        for (uint32_t i0 = j; i0 < Dmain; i0 += 8u * KB) {
            uint16_t h[KB];
#pragma unroll
            for (uint32_t k = 0; k < KB; ++k) h[k] = row[i0 + 8u * k < Dmain ? i0 + 8u * k : 0u];
#pragma unroll
            for (uint32_t k = 0; k < KB; ++k)
                if (i0 - j + 8u * k < Dmain) acc = rp_add<IP>(acc, sq[i0 + 8u * k], rp_widen<RAW>(h[k]));
        }
    } else {
        const bool b0 = (j & 1u) != 0u, b1 = (j & 2u) != 0u, b2 = (j & 4u) != 0u;
        const uint32_t sel = b0 ? 0x03020706u : 0x05040100u;
        auto load_spans = [&](uint4* v, uint32_t e0) {
#pragma unroll
            for (uint32_t s = 0; s < kRpSpans; ++s) {
                const uint32_t e = e0 + 64u * s + 8u * j;
                v[s] = rp_load16h(row + (e + 8u <= Dmain ? e : 0u));
            }
        };
        uint4 v[kRpSpans], nx[kRpSpans];
        if (Dmain) load_spans(v, 0u);
        for (uint32_t e0 = 0; e0 < Dmain; e0 += 64u * kRpSpans) {
            load_spans(nx, e0 + 64u * kRpSpans); // the next spans travel while these are consumed
#pragma unroll
            for (uint32_t s = 0; s < kRpSpans; ++s) {
                uint32_t d[4] = {v[s].x, v[s].y, v[s].z, v[s].w};
                rp_transpose8x8(d, b0, b1, b2, sel);
#pragma unroll
                for (uint32_t m = 0; m < 8u; ++m) {
                    const uint32_t c0 = e0 + 64u * s + 8u * m; // chunk of eight elements (wave-uniform)
                    if (c0 < Dmain) acc = rp_add<IP>(acc, sq[c0 + j], (m & 1u) ? rp_widen_hi<RAW>(d[m >> 1]) : rp_widen_lo<RAW>(d[m >> 1]));
                }
            }
#pragma unroll
            for (uint32_t s = 0; s < kRpSpans; ++s) v[s] = nx[s];
        }
    }
    float sum = 0.0f;
    if (Dmain) {
        sum = -0.0f;
#pragma unroll
        for (uint32_t l = 0; l < 8u; ++l) sum = sum + __shfl(acc, (int)(base | l));
    }
    for (uint32_t i = Dmain; i < dim; ++i) sum = rp_add<IP>(sum, sq[i], rp_widen<RAW>(row[i]));
    return sum;
}

// The score of raw row `id` (rows of dim elements of RAW at `raw`) against the query at sq, on the eight lanes of a group: the one
// entry both kernels call.  act false (no candidate in this group, or id >= n_raw): row 0 stands in, read and discarded — the caller
// writes the NaN 0x7fc00000 or nothing.  n_raw >= 1.
template <bool IP, int RAW>
__device__ __forceinline__ float rp_score_row(const void* raw, uint64_t id, bool act, const float* sq, uint32_t dim, uint32_t j, uint32_t base,
                                              bool by_element) {
    const size_t off = act ? (size_t)id * dim : (size_t)0;
    if constexpr (RAW == kRawF32) return rp_score32<IP>((const float*)raw + off, sq, dim, j, base);
    else return rp_score16<IP, RAW>((const uint16_t*)raw + off, sq, dim, j, base, by_element);
}

} // namespace rbq
