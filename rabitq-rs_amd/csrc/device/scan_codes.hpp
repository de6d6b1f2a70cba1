// scan_codes.hpp — what the scan kernels do to ONE vector's codes (gfx950, wave64): the sign-code lookups through the LDS LUT (k_scan,
// k_scanw, k_mstg_refine), the ex-code dot products of a refine round that only the scans use (ex_dot_units / ex_dot_all, which
// k_select_mfma shares, are in kernels.hpp), and the refined distance both scans form from them.
#pragma once
#include "kernels.hpp"

namespace rbq {

// LUT pointer in the LDS address space, formed from a plain integer offset.  A pointer derived from the
// `extern __shared__` symbol carries a link-time relocation that hipcc adds with one v_add_u32 PER LOOKUP
// (`v_add_u32 v, 0, v` after linking); an integer-derived address lets the codebook offset fold into the
// ds_read_u8 immediate.  k_scan keeps its LUT at LDS byte 0 and traps if the dynamic region is not there.
typedef const __attribute__((address_space(3))) uint8_t* lds_lut_ptr;

// 8 nibble lookups of one little-endian code dword; table p+16*m serves nibble m.  The empty asm pins the
// running sum so the integer adds are not re-associated into one end-of-block reduction (which made hipcc
// keep, and spill, every ds_read result).
__device__ __forceinline__ void look8(uint32_t& acc, uint32_t x, lds_lut_ptr p) {
    uint32_t s = p[x & 15u];
    s += p[16 + ((x >> 4) & 15u)];
    s += p[32 + ((x >> 8) & 15u)];
    s += p[48 + ((x >> 12) & 15u)];
    s += p[64 + ((x >> 16) & 15u)];
    s += p[80 + ((x >> 20) & 15u)];
    s += p[96 + ((x >> 24) & 15u)];
    s += p[112 + (x >> 28)];
    acc += s;
    asm("" : "+v"(acc));
}

// Register image of one vector's sign code (lane l32 of a block): a ROLLING window of kCodeWin 16-byte granules
// (+ the optional 8-byte tail).  The first window is requested with the factor rows; granule g + kCodeWin is
// requested when granule g has been consumed, so at most kCodeWin + 1 granules are live — the full image
// (30 registers at D = 960) made the lookup phase the register peak of the kernel.
// (a window of one granule still spilled in the instantiations at their register limit)
constexpr int kCodeWin = 2;
template <int DT>
struct CodeRegs {
    static constexpr int G = DT >> 7;                         // full granules
    static constexpr int W = G < kCodeWin ? (G ? G : 1) : kCodeWin;
    uint4 x[W];
    uint2 tail;
};

template <int DT>
__device__ __forceinline__ void load_codes(CodeRegs<DT>& c, const uint8_t* __restrict__ blk, uint32_t l32) {
    const uint4* cp = reinterpret_cast<const uint4*>(blk) + l32;
#pragma unroll
    for (int g = 0; g < CodeRegs<DT>::W && g < (DT >> 7); ++g) c.x[g] = cp[g * 32];
    if (DT & 64) {
        // (the lane's byte offset is formed HERE, behind an empty asm: hoisted out of the tile loop it is a 64-bit loop invariant per
        // lane, and in the instantiations that sit at their register limit that pair was the value hipcc chose to spill — a scratch
        // reload with its s_waitcnt vmcnt(0) between the code loads of every tile)
        uint32_t off = l32 * 8u;
        asm volatile("" : "+v"(off));
        c.tail = *reinterpret_cast<const uint2*>(blk + (DT >> 7) * 512 + off);
    }
}

template <int DT>
__device__ __forceinline__ uint32_t lookup_codes(CodeRegs<DT>& c, const uint8_t* __restrict__ blk, uint32_t l32, lds_lut_ptr lut) {
    constexpr int G = DT >> 7, W = CodeRegs<DT>::W;
    uint32_t off = l32 * 16u; // (formed here, behind an empty asm, not hoisted: see load_codes)
    asm volatile("" : "+v"(off));
    const uint4* cp = reinterpret_cast<const uint4*>(blk + off);
    uint32_t acc = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint4 x = c.x[g % W];
        if (g + W < G) c.x[g % W] = cp[(g + W) * 32];
        look8(acc, x.x, lut + g * 512);
        look8(acc, x.y, lut + g * 512 + 128);
        look8(acc, x.z, lut + g * 512 + 256);
        look8(acc, x.w, lut + g * 512 + 384);
    }
    if (DT & 64) {
        look8(acc, c.tail.x, lut + G * 512);
        look8(acc, c.tail.y, lut + G * 512 + 128);
    }
    return acc;
}

// Measured and not kept (k_scanw below top_k 64; records: profiles/lds_pipeline): this sum software-pipelined over the code dwords.  look8's
// pin makes the wave drain the LDS queue once per dword (8 ds_read_u8, `s_waitcnt lgkmcnt(6) (4) (2) (0)` between the adds, the next
// dword's reads behind that lgkmcnt(0)): 29 full drains per tile at D = 960.  With the reads of stage t + 1 issued before the sums of
// stage t (the pin kept, on the accumulator alone) the ISA had no drain left and only counted waits — and a wave alone on its SIMD took
// LONGER per tile: 5010 cycles with stages of half a dword, 4934 with whole dwords, against 4573; queries/s did not differ.  The eight
// reads of a dword already overlap each other; what the drain exposes is less than what the staging adds.

// generic (runtime Dc) path: no register prefetch
__device__ __forceinline__ uint32_t accumulate_block_rt(const uint8_t* __restrict__ blk, lds_lut_ptr lut,
                                                        uint32_t l32, uint32_t Dc) {
    const uint32_t G16 = Dc >> 7;
    const uint4* cp = reinterpret_cast<const uint4*>(blk) + l32;
    uint32_t acc = 0;
    for (uint32_t g = 0; g < G16; ++g) {
        uint4 x = cp[g * 32];
        look8(acc, x.x, lut + g * 512);
        look8(acc, x.y, lut + g * 512 + 128);
        look8(acc, x.z, lut + g * 512 + 256);
        look8(acc, x.w, lut + g * 512 + 384);
    }
    if (Dc & 64u) {
        uint2 y = *(reinterpret_cast<const uint2*>(blk + G16 * 512) + l32);
        look8(acc, y.x, lut + G16 * 512);
        look8(acc, y.y, lut + G16 * 512 + 128);
    }
    return acc;
}

// workgroup barrier that only drains LDS traffic: prefetched global loads stay in flight across it
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Distance of a candidate refined with its ex codes, in the reference's operation order: ip = the 1-bit inner
// product of the tile step, s = the ex-code dot product, fa / fr = the vector's f_add_ex / f_rescale_ex, gadd = its list's g_add.
// One statement per rounding (the build has -ffp-contract=off; nothing here may fuse or re-associate).
__device__ __forceinline__ float refined_distance(float scale, float ip, float s, float kbx, float fa, float gadd, float fr) {
    float tt2 = scale * ip;
    tt2 = tt2 + s;
    tt2 = tt2 + kbx;
    const float a = fa + gadd;
    const float m = fr * tt2;
    return a + m;
}

// (ex_dot_units<EX> and group16_reduce: kernels.hpp — k_select_mfma evaluates head vectors with them too)
// (ex_load_all / ex_dot_all — the same arithmetic with all units of a vector requested before the first is decoded: kernels.hpp)
// Two vectors at once: every query value is read from LDS once and feeds two independent FMA chains in the
// reference's order (used when a vector's ex codes fit ONE 128-bit unit per lane, i.e. small dimensions, where a
// refine round is pure memory latency and twice the survivors per round halve the rounds).
template <int EX>
__device__ __forceinline__ void ex_dot_pair1(const uint4& u0, const uint4& u1, const float* sq, uint32_t gl, uint32_t ncodes,
                                             float& s0, float& s1) {
    constexpr int CPU = 128 / EX;
    constexpr uint32_t mask = (1u << EX) - 1u;
    const uint32_t w0[5] = {u0.x, u0.y, u0.z, u0.w, 0u}, w1[5] = {u1.x, u1.y, u1.z, u1.w, 0u};
    const float* qj = sq + gl;
    s0 = 0.0f; s1 = 0.0f;
#pragma unroll
    for (int k = 0; k < CPU; ++k) {
        if ((uint32_t)k < ncodes) { // wave-uniform: D/16 codes per lane
            const int bit = k * EX, idx = bit >> 5, sh = bit & 31;
            uint32_t c0, c1;
            if (sh + EX <= 32) { c0 = (w0[idx] >> sh) & mask; c1 = (w1[idx] >> sh) & mask; }
            else {
                c0 = ((w0[idx] >> sh) | (w0[idx + 1] << (32 - sh))) & mask;
                c1 = ((w1[idx] >> sh) | (w1[idx + 1] << (32 - sh))) & mask;
            }
            const float qv = qj[16 * k];
            s0 = fmaf((float)c0, qv, s0);
            s1 = fmaf((float)c1, qv, s1);
        }
    }
}
// The same for vectors whose codes span NU units per lane (NU = 2, 3: D = 768 / 960 at 6 bits), on PACKED f32 FMAs: the two
// survivors' chains are the two halves of one v_pk_fma_f32 per code (each half is the reference's own fused
// multiply-add, in its own order), the query value is read from LDS once for both.  Per code: 2 extractions, 2 converts,
// 1 LDS read, 1 packed FMA instead of 2 x (extract, convert, LDS read, FMA).  Used for top_k >= 64, where most refined
// candidates enter the top-k and a refine round of twice the size is not wasted work.
// EVERY unit of both vectors is requested before the first one is decoded: one memory round trip per refine round.  (A loop
// that kept one unit in flight was rotated by hipcc so that each iteration waited for its own loads — NU dependent round trips
// per round, 3 at D = 960: the ISA showed `global_load_dwordx4` at the loop top followed by `s_waitcnt vmcnt(0)`.)  The units
// are decoded one after the other; the empty asm between them keeps the LDS reads of unit j + 1 from being hoisted above
// unit j (all 3 x 21 query values alive: spills).
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kPairPin = 4; // query values (LDS reads) in flight per decode stretch
template <int EX, int NU>
__device__ __forceinline__ void ex_dot_pair_all(const uint4* __restrict__ p0, const uint4* __restrict__ p1, const float* sq, uint32_t gl,
                                                float& s0, float& s1) {
    constexpr int CPU = 128 / EX;
    constexpr uint32_t mask = (1u << EX) - 1u;
    uint4 a[NU], b[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) { a[j] = p0[j * 16]; b[j] = p1[j * 16]; }
    f32x2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const uint32_t w0[5] = {a[j].x, a[j].y, a[j].z, a[j].w, 0u}, w1[5] = {b[j].x, b[j].y, b[j].z, b[j].w, 0u};
        const float* qj = sq + j * CPU * 16 + gl;
#pragma unroll
        for (int k = 0; k < CPU; ++k) {
            const int bit = k * EX, idx = bit >> 5, sh = bit & 31;
            uint32_t c0, c1;
            if (sh + EX <= 32) { c0 = (w0[idx] >> sh) & mask; c1 = (w1[idx] >> sh) & mask; }
            else {
                c0 = ((w0[idx] >> sh) | (w0[idx + 1] << (32 - sh))) & mask;
                c1 = ((w1[idx] >> sh) | (w1[idx + 1] << (32 - sh))) & mask;
            }
            const float qv = qj[16 * k]; // (zero beyond D: the padded code slots are zero as well, 0 * 0 + s == s)
            const f32x2 cf = {(float)c0, (float)c1}, qq = {qv, qv};
            acc = __builtin_elementwise_fma(cf, qq, acc);
            if (k % kPairPin == kPairPin - 1 || k == CPU - 1) asm volatile("" : "+v"(acc) :: "memory");
        }
    }
    s0 = acc.x; s1 = acc.y;
}

// Decode halves of the above for callers that request the units themselves and do other work while they are in flight
// (k_scanw): `a` / `b` = the NU units of the two vectors; NCODES = D / 16 codes per lane (the tail of the last unit is zero padding
// and is not decoded).
template <int EX, int NU, int NCODES>
__device__ __forceinline__ void ex_dot_pair_regs(const uint4* a, const uint4* b, const float* sq, uint32_t gl, float& s0, float& s1) {
    constexpr int CPU = 128 / EX;
    constexpr uint32_t mask = (1u << EX) - 1u;
    f32x2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        uint4 wa = a[j], wb = b[j];
        const float* qj = sq + j * CPU * 16 + gl;
#pragma unroll
        for (int k = 0; k < CPU; ++k) {
            if (j * CPU + k < NCODES) {
                const uint32_t w0[5] = {wa.x, wa.y, wa.z, wa.w, 0u}, w1[5] = {wb.x, wb.y, wb.z, wb.w, 0u};
                const int bit = k * EX, idx = bit >> 5, sh = bit & 31;
                uint32_t c0, c1;
                if (sh + EX <= 32) { c0 = (w0[idx] >> sh) & mask; c1 = (w1[idx] >> sh) & mask; }
                else {
                    c0 = ((w0[idx] >> sh) | (w0[idx + 1] << (32 - sh))) & mask;
                    c1 = ((w1[idx] >> sh) | (w1[idx + 1] << (32 - sh))) & mask;
                }
                const float qv = qj[16 * k];
                const f32x2 cf = {(float)c0, (float)c1}, qq = {qv, qv};
                acc = __builtin_elementwise_fma(cf, qq, acc);
                // the FMA chain is serial, so the scheduler hoists the (independent) decode of every later code above it — a
                // hundred live registers; passing the code words through the pin as well keeps the decode within a stretch
                if (k % kPairPin == kPairPin - 1 || k == CPU - 1 || j * CPU + k == NCODES - 1)
                    asm volatile("" : "+v"(acc), "+v"(wa.x), "+v"(wa.y), "+v"(wa.z), "+v"(wa.w), "+v"(wb.x), "+v"(wb.y), "+v"(wb.z), "+v"(wb.w) :: "memory");
            }
        }
    }
    s0 = acc.x; s1 = acc.y;
}
// AHEAD > 0 (k_scanw below top_k 64): in the plain form (AHEAD = 0, below) the pin's "memory" clobber keeps the query reads of a stretch
// behind the previous stretch's FMAs, and the wave drains the LDS queue about every second FMA (one or two ds_read2_b32 in flight, then
// `s_waitcnt lgkmcnt(0)`): 27 drains per candidate at D = 960.  Here code c of the vector reads sq[gl + 16 c] (the units are
// contiguous in c), the codes are cut into stretches of kPairPin in index order across the unit boundaries, and the query values of
// stretch s + AHEAD are requested between the pins that end stretches s - 1 and s: a read in front of a "memory" clobber stays there.
// With AHEAD = 2 a whole stretch of reads is outstanding behind the ones an FMA waits for, wherever the scheduler puts the requests
// between two pins; with AHEAD = 1 (four registers less) it put them behind the stretch's second FMA: half a stretch.  The values are
// not operands of the pin (an asm operand is a use).  The FMA chain is the same: one fmaf per code, codes in index order.
template <int EX, int NU, int NCODES, int AHEAD = 0>
__device__ __forceinline__ float ex_dot_one_regs(const uint4* a, const float* sq, uint32_t gl) {
    constexpr int CPU = 128 / EX;
    constexpr uint32_t mask = (1u << EX) - 1u;
    float acc = 0.0f;
    if constexpr (AHEAD > 0) {
        constexpr int NS = (NCODES + kPairPin - 1) / kPairPin;
        const float* qb = sq + gl;
        float qv[AHEAD + 1][kPairPin];
#pragma unroll
        for (int t = 0; t < AHEAD * kPairPin; ++t) qv[t / kPairPin][t % kPairPin] = t < NCODES ? qb[16 * t] : 0.0f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int t = 0; t < kPairPin; ++t) {
                const int c = (s + AHEAD) * kPairPin + t;
                if (c < NCODES) qv[(s + AHEAD) % (AHEAD + 1)][t] = qb[16 * c];
            }
#pragma unroll
            for (int t = 0; t < kPairPin; ++t) {
                const int c = s * kPairPin + t;
                if (c < NCODES) {
                    const int j = c / CPU, bit = (c % CPU) * EX, idx = bit >> 5, sh = bit & 31;
                    const uint32_t w0[5] = {a[j].x, a[j].y, a[j].z, a[j].w, 0u};
                    uint32_t c0;
                    if (sh + EX <= 32) c0 = (w0[idx] >> sh) & mask;
                    else c0 = ((w0[idx] >> sh) | (w0[idx + 1] << (32 - sh))) & mask;
                    acc = fmaf((float)c0, qv[s % (AHEAD + 1)][t], acc);
                }
            }
            asm volatile("" : "+v"(acc) :: "memory");
        }
        return acc;
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const uint32_t w0[5] = {a[j].x, a[j].y, a[j].z, a[j].w, 0u};
        const float* qj = sq + j * CPU * 16 + gl;
#pragma unroll
        for (int k = 0; k < CPU; ++k) {
            if (j * CPU + k < NCODES) {
                const int bit = k * EX, idx = bit >> 5, sh = bit & 31;
                uint32_t c0;
                if (sh + EX <= 32) c0 = (w0[idx] >> sh) & mask;
                else c0 = ((w0[idx] >> sh) | (w0[idx + 1] << (32 - sh))) & mask;
                acc = fmaf((float)c0, qj[16 * k], acc);
                if (k % kPairPin == kPairPin - 1 || k == CPU - 1 || j * CPU + k == NCODES - 1) asm volatile("" : "+v"(acc) :: "memory");
            }
        }
    }
    return acc;
}

} // namespace rbq
