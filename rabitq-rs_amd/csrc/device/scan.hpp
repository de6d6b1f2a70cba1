// scan.hpp — k_scan, the roofline kernel of the IVF+RaBitQ query path (gfx950, wave64).
//
// Reference semantics: search_cluster_v2_batched (src/ivf.rs:1901-2129) over the probed lists of one
// query, i.e. accumulate_batch (src/simd.rs:972-1184) + compute_batch_distances_u16 (:2090-2140) +
// lower-bound pruning + ip_packed_ex{2,6}_f32 (:1835-1915) + BinaryHeap top-k (src/ivf.rs:904-931).
//
// One workgroup = one query, with fixed wave roles:
//   waves 0..NS-1 "scanners": consume the query's block stream (k_select_mfma: probe order, block order inside a
//             list, each entry with its precomputed block-level lower bound) in fill steps (one lane per entry:
//             bound vs threshold -> live-block FIFO) and tile steps (2*NS live blocks, lane = vector: codes ->
//             LDS LUT lookups -> fused epilogue); survivors (lb < T) are published (mask, lb, ip, est, slot) to a
//             double-buffered LDS queue.
//   wave NS   "replay wave": compacts the previous tile's survivors in stream order, refines lazily (only
//             survivors still below the true threshold, 16 lanes per survivor over a lane-major copy of the ex
//             codes) and replays them through the reference's exact prune/push/pop loop while the scanners are
//             already on the next tile; publishes T.  The top-k lives in the wave's registers: a sorted run while
//             all distances are distinct, the Rust-BinaryHeap-faithful RegHeap after an in-kernel restart
//             otherwise (see SortedTop).
// Exactness: scanners prune with a STALE threshold T.  T only ever shrinks, so `lb >= T_stale` implies the
// reference (whose threshold at that moment is <= T_stale) skipped the candidate too; everything else is
// re-tested by the replay wave against the true running threshold, in stream order.  ids therefore equal
// the sequential CPU path bit for bit.  Tiles with more than kLightMax survivors (the first probed lists,
// where T is still loose) run synchronously, software-pipelined: the scanners' groups refine batch r+1 while
// the replay wave replays batch r.
#pragma once
#include "kernels.hpp"

namespace rbq {

#ifndef RBQ_SCAN_WAVES
#define RBQ_SCAN_WAVES 5    // launch-bounds occupancy target (waves per SIMD): 96 VGPRs, room for a fifth wave of another kernel
#endif
#ifndef RBQ_LIGHT_MAX
#define RBQ_LIGHT_MAX 12
#endif
#ifndef RBQ_PIN_MODE
#define RBQ_PIN_MODE 1
#endif
constexpr uint32_t kLightMax = RBQ_LIGHT_MAX;   // tiles with more survivors than this run synchronously
constexpr uint32_t kBatchDone = 0xffffffffu;

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
#if RBQ_PIN_MODE == 0
    asm volatile("" : "+v"(acc));
#elif RBQ_PIN_MODE == 1
    asm("" : "+v"(acc));
#endif
}

// Register image of one vector's sign code (lane l32 of a block): a ROLLING window of kCodeWin 16-byte granules
// (+ the optional 8-byte tail).  The first window is requested with the factor rows; granule g + kCodeWin is
// requested when granule g has been consumed, so at most kCodeWin + 1 granules are live — the full image
// (30 registers at D = 960) made the lookup phase the register peak of the kernel.
#ifndef RBQ_CODE_WIN
#define RBQ_CODE_WIN 2
#endif
// per-lane byte offsets of the code loads pass through an empty asm where they are used (see load_codes)
#ifndef RBQ_ANTIHOIST
#define RBQ_ANTIHOIST 1
#endif
#if RBQ_ANTIHOIST == 1
#define RBQ_OPAQUE(x) asm volatile("" : "+v"(x))
#define RBQ_OPAQUE2(x) asm volatile("" : "+v"(x))
#elif RBQ_ANTIHOIST == 2
#define RBQ_OPAQUE(x) asm("" : "+v"(x))
#define RBQ_OPAQUE2(x) asm("" : "+v"(x))
#elif RBQ_ANTIHOIST == 3
#define RBQ_OPAQUE(x) asm volatile("" : "+v"(x))
#define RBQ_OPAQUE2(x)
#else
#define RBQ_OPAQUE(x)
#define RBQ_OPAQUE2(x)
#endif
constexpr int kCodeWin = RBQ_CODE_WIN;
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
        RBQ_OPAQUE(off);
        c.tail = *reinterpret_cast<const uint2*>(blk + (DT >> 7) * 512 + off);
    }
}

template <int DT>
__device__ __forceinline__ uint32_t lookup_codes(CodeRegs<DT>& c, const uint8_t* __restrict__ blk, uint32_t l32, lds_lut_ptr lut) {
    constexpr int G = DT >> 7, W = CodeRegs<DT>::W;
    uint32_t off = l32 * 16u; // (formed here, not hoisted: see load_codes)
    RBQ_OPAQUE2(off);
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

// ---- Rust std BinaryHeap<HeapEntry> on LDS arrays (max-heap on total_cmp(distance)) -----------------------
struct LdsHeap {
    float* d;
    uint32_t* s;
    uint32_t len;
    __device__ __forceinline__ void sift_up(uint32_t pos, float ed, uint32_t es) {
        const int ke = total_key(ed);
        while (pos > 0) {
            const uint32_t parent = (pos - 1) >> 1;
            if (ke <= total_key(d[parent])) break;
            d[pos] = d[parent];
            s[pos] = s[parent];
            pos = parent;
        }
        d[pos] = ed;
        s[pos] = es;
    }
    __device__ __forceinline__ void push(float dist, uint32_t slot) { sift_up(len++, dist, slot); }
    __device__ __forceinline__ void pop() { // last -> root, sift_down_to_bottom(0), sift_up
        --len;
        if (len == 0) return;
        const float ed = d[len];
        const uint32_t es = s[len];
        const uint32_t end = len;
        uint32_t p = 0, child = 1;
        while (end >= 2 && child <= end - 2) {
            child += (total_key(d[child]) <= total_key(d[child + 1])) ? 1u : 0u;
            d[p] = d[child];
            s[p] = s[child];
            p = child;
            child = 2 * p + 1;
        }
        if (child == end - 1) {
            d[p] = d[child];
            s[p] = s[child];
            p = child;
        }
        sift_up(p, ed, es);
    }
    __device__ __forceinline__ void into_sorted() { // into_sorted_vec: swap(0,end); sift_down_range(0,end)
        uint32_t end = len;
        while (end > 1) {
            --end;
            const float ed = d[end];
            const uint32_t es = s[end];
            d[end] = d[0];
            s[end] = s[0];
            const int ke = total_key(ed);
            uint32_t p = 0, child = 1;
            bool placed = false;
            while (end >= 2 && child <= end - 2) {
                child += (total_key(d[child]) <= total_key(d[child + 1])) ? 1u : 0u;
                if (ke >= total_key(d[child])) { placed = true; break; }
                d[p] = d[child];
                s[p] = s[child];
                p = child;
                child = 2 * p + 1;
            }
            if (!placed && child == end - 1 && ke < total_key(d[child])) {
                d[p] = d[child];
                s[p] = s[child];
                p = child;
            }
            d[p] = ed;
            s[p] = es;
        }
    }
};

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
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int EX, int NU>
__device__ __forceinline__ void ex_dot_pair_units(const uint4* __restrict__ p0, const uint4* __restrict__ p1, const float* sq, uint32_t gl,
                                                  float& s0, float& s1) {
    constexpr int CPU = 128 / EX;
    constexpr uint32_t mask = (1u << EX) - 1u;
    f32x2 acc = {0.0f, 0.0f};
    uint4 c0v = p0[0], c1v = p1[0]; // unit j of both vectors in registers, unit j + 1 in flight (all NU units of both: spills)
#pragma unroll 1
    for (int j = 0; j < NU; ++j) { // (a real loop: fully unrolled, hipcc keeps all 3 x 21 query values of a vector pair alive)
        const int jn = j + 1 < NU ? j + 1 : j;
        const uint4 n0v = p0[jn * 16], n1v = p1[jn * 16];
        const uint32_t w0[5] = {c0v.x, c0v.y, c0v.z, c0v.w, 0u}, w1[5] = {c1v.x, c1v.y, c1v.z, c1v.w, 0u};
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
        }
        c0v = n0v; c1v = n1v;
    }
    s0 = acc.x; s1 = acc.y;
}

// The same pair refine with EVERY unit of both vectors requested before the first one is decoded: one memory round trip per
// refine round.  (ex_dot_pair_units above keeps one unit in flight, but hipcc rotates its loop so that each iteration waits
// for its own loads — NU dependent round trips per round, 3 at D = 960: the ISA showed `global_load_dwordx4` at the loop top
// followed by `s_waitcnt vmcnt(0)`.)  The units are decoded one after the other; the empty asm between them keeps the LDS
// reads of unit j + 1 from being hoisted above unit j (all 3 x 21 query values alive: spills).
#ifndef RBQ_PAIR_PIN
#define RBQ_PAIR_PIN 4 // query values (LDS reads) in flight per decode stretch
#endif
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
            if (k % RBQ_PAIR_PIN == RBQ_PAIR_PIN - 1 || k == CPU - 1) asm volatile("" : "+v"(acc) :: "memory");
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
                if (k % RBQ_PAIR_PIN == RBQ_PAIR_PIN - 1 || k == CPU - 1 || j * CPU + k == NCODES - 1)
                    asm volatile("" : "+v"(acc), "+v"(wa.x), "+v"(wa.y), "+v"(wa.z), "+v"(wa.w), "+v"(wb.x), "+v"(wb.y), "+v"(wb.z), "+v"(wb.w) :: "memory");
            }
        }
    }
    s0 = acc.x; s1 = acc.y;
}
template <int EX, int NU, int NCODES>
__device__ __forceinline__ float ex_dot_one_regs(const uint4* a, const float* sq, uint32_t gl) {
    constexpr int CPU = 128 / EX;
    constexpr uint32_t mask = (1u << EX) - 1u;
    float acc = 0.0f;
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
                if (k % RBQ_PAIR_PIN == RBQ_PAIR_PIN - 1 || k == CPU - 1 || j * CPU + k == NCODES - 1) asm volatile("" : "+v"(acc) :: "memory");
            }
        }
    }
    return acc;
}

// ---- the same BinaryHeap held in the replay wave's registers ------------------------------------------------
// Entry i lives in lane i % 64 of register i / 64; TR registers hold 64*TR entries (the heap is one entry over top_k
// between a push and the pop that follows, so top_k <= 64*TR - 1: 63 with one register, 255 with four).
// All indices and values are wave-uniform, so every access is a v_readlane/v_writelane (a few cycles)
// instead of a dependent LDS round trip.  Register 0 is the pair (hd, hs); registers 1..TR-1 are elements of two
// vector values (element 0 unused) — vector elements with compile-time indices stay in VGPRs, a plain array ended up
// in scratch.  The sorted run (SortedRun below) is a second view of the same registers; only one is live at a time.
struct HeapOps {
    // every index is wave-uniform; readfirstlane makes that explicit so that hipcc emits a plain v_readlane instead of
    // a waterfall loop
    static __device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    static __device__ __forceinline__ int key(int bits) { return bits ^ (int)(((uint32_t)(bits >> 31)) >> 1); }
};
template <int TR>
struct RegHeap : HeapOps {
    typedef int VI __attribute__((ext_vector_type(TR)));
    typedef uint32_t VU __attribute__((ext_vector_type(TR)));
    int hd;      // distance bits of entry `lane`
    uint32_t hs; // slot of entry `lane`
    VI xd;       // entries 64r + lane, r = 1..TR-1
    VU xs;
    uint32_t len;
    __device__ __forceinline__ int d_at(uint32_t i) const {
        const uint32_t r = uni(i >> 6);
        int v = hd;
#pragma unroll
        for (int k = 1; k < TR; ++k) v = r == (uint32_t)k ? xd[k] : v;
        return __builtin_amdgcn_readlane(v, (int)uni(i & 63u));
    }
    __device__ __forceinline__ uint32_t s_at(uint32_t i) const {
        const uint32_t r = uni(i >> 6);
        uint32_t v = hs;
#pragma unroll
        for (int k = 1; k < TR; ++k) v = r == (uint32_t)k ? xs[k] : v;
        return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)uni(i & 63u));
    }
    __device__ __forceinline__ void set(uint32_t i, int d, uint32_t s) { // v_writelane as compare+select
        const uint32_t r = uni(i >> 6);
        const bool me = (__lane_id() == uni(i & 63u));
        const bool m0 = me && r == 0u;
        hd = m0 ? d : hd;
        hs = m0 ? s : hs;
#pragma unroll
        for (int k = 1; k < TR; ++k) {
            const bool mk = me && r == (uint32_t)k;
            xd[k] = mk ? d : xd[k];
            xs[k] = mk ? s : xs[k];
        }
    }
    __device__ __forceinline__ void sift_up(uint32_t pos, int ed, uint32_t es) {
        const int ke = key(ed);
        pos = uni(pos);
        while (pos > 0) {
            const uint32_t parent = uni((pos - 1) >> 1);
            const int pd = d_at(parent);
            if (ke <= key(pd)) break;
            set(pos, pd, s_at(parent));
            pos = parent;
        }
        set(pos, ed, es);
    }
    __device__ __forceinline__ void push(int dbits, uint32_t slot) {
        const uint32_t p = uni(len);
        len = p + 1;
        sift_up(p, dbits, slot);
    }
    __device__ __forceinline__ void pop() {
        len = uni(len - 1);
        if (len == 0) return;
        const int ed = d_at(len);
        const uint32_t es = s_at(len);
        const uint32_t end = len;
        uint32_t p = 0, child = 1;
        while (end >= 2 && child <= end - 2) {
            const int c0 = d_at(child), c1 = d_at(child + 1);
            const bool right = key(c0) <= key(c1);
            child = uni(child + (right ? 1u : 0u));
            set(p, right ? c1 : c0, s_at(child));
            p = child;
            child = uni(2 * p + 1);
        }
        if (child == end - 1) {
            set(p, d_at(child), s_at(child));
            p = child;
        }
        sift_up(p, ed, es);
    }
};

// ---- tie-free fast path of the same top-k --------------------------------------------------------------------
// As long as no two distances in the heap are bit-identical, the reference's result does not depend on the
// layout of its BinaryHeap: pop evicts THE maximum and into_sorted_vec has one possible order.  Any equality the
// fast path meets reports a tie; the query is then re-run from its first block with the exact BinaryHeap emulation
// (RegHeap while top_k < 64*TR, LdsHeap above).
//
// RankRun (TR > 1: 64 <= top_k <= 256, the reference's own benchmark setting is 100): the top-k is a SORTED RUN of
// KEYS (HeapOps::key of the distance bits: a signed-integer image of total_cmp, its own inverse) in the RegHeap's
// registers, entry i in lane i % 64 of register i / 64, empty lanes = kHigh.  A whole refine batch (up to 64 candidates
// in stream order, lane j = candidate j) is merged in ONE data-parallel step instead of one candidate after the other —
// at top_k = 100 most evaluated candidates enter the top-k, and a serial insertion per candidate (~700 cycles of
// dependent scalar/DPP work each on a SIMD shared with the refining waves) was two thirds of the kernel.
//
// The reference's loop over the batch is, with U_j = run + candidates accepted before j and t_j = k-th smallest of U_j
// (+inf while |U_j| < k):   skip j if lb_j >= t_j;  drop j if d_j is not finite;  accept j iff d_j < t_j (then the
// maximum leaves when |U| > k).  Its final top-k F is the k smallest of run + A (A = accepted candidates).
// Claim: F = F' := the k smallest of  run + C,  C = ALL finite candidates of the batch, provided every candidate o in F'
// with lb_o >= d_o ("odd": lower bound not below the refined distance) has lb_o < m' := max F'.
// Proof (|run + C| >= k; otherwise every threshold is +inf, nothing is skipped, rejected or evicted, and F = F' = all):
// U_j is a subset of run + C, so its k-th smallest is not below that of run + C:  t_j >= m'  for every j.  Take a
// candidate s in F': d_s <= m' <= t_s.  If s is not odd, lb_s < d_s <= t_s: the reference evaluates it; if it is odd,
// lb_s < m' <= t_s by the proviso: evaluated as well.  It then accepts s unless d_s == t_s — an equal key inside
// run + C, reported as a tie (below).  So F' is a subset of run + A, which is a subset of run + C; being the k smallest of
// the larger set, F' is also the k smallest of run + A, i.e. F.  No acceptance decision, no thresholds — one merge:
//     G(u) = #{elements of run + candidates above u}:  run entries: position from the top + #{candidates > u};
//     candidates: #{run entries > x} + #{candidates > x};  with E = max(0, |run| + |candidates| - k), u stays iff
//     G(u) >= E, and its new position from the top is G(u) - E.  One scatter through LDS.
// When the proviso fails (or diagnostics want the exact c_skip/c_ext/c_est, which need the thresholds themselves) the
// batch is decided by the serial simulation below and merged the same way.
// Ties (the reference's result then depends on the layout of its heap; any of these reports a tie): two candidates with
// equal keys get the same G and are scattered to the same position, which leaves another position unwritten (lds_k is
// pre-filled with kHigh); a candidate equal to a run key lands next to it (neighbour check after the reload); an element
// that leaves with the same key as the new maximum (checked against the old registers).  Equal keys that both leave do
// not matter to the reference either.
template <int TR>
struct RankRun {
    typedef RegHeap<TR> H;
    static constexpr int kHigh = 0x7fffffff; // key of a NaN pattern: never inserted (non-finite distances are dropped)
    static constexpr int kLow = (int)0x80000000;
    static __device__ __forceinline__ void clear(H& h) { h.hd = kHigh; h.hs = 0u; h.xd = kHigh; h.xs = 0u; h.len = 0u; }
    static __device__ __forceinline__ int wave_max(int m) {
        int t;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x111, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x112, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x114, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x118, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x142, 0xa, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x143, 0xc, 0xf, false); m = t > m ? t : m;
        return __builtin_amdgcn_readlane(m, 63);
    }
    // Merge the batch `mt` (lane j: lower-bound bits v_lb, refined distance bits v_d, slot v_s) into the run.  `serial`
    // forces the serial decision (exact c_skip/c_ext/c_est: diagnostics).  dk_bits <- bits of the k-th distance once the
    // run is full.  lds_k/lds_s: scratch for top_k entries.  Returns true if an equal key was met.
    // lazy / amb_min: LAZY TIES (k_scanw).  Equal keys do not end the fast path on the spot: they are ordered by a fixed rule (run
    // entries below candidates, candidates by lane) and merged like any others; what is recorded is the one thing that can make
    // the reference's RESULT depend on the layout of its heap later on — an element that LEAVES (or is turned away) with the key of
    // the maximum that stays: amb_min = the smallest such key.  See k_scanw's final check for why that, plus a look at the final
    // run for equal neighbours, decides exactly the queries that need the BinaryHeap emulation.
    static __device__ __forceinline__ bool merge_batch(H& h, uint32_t top_k, unsigned long long mt, int v_lb, int v_d, uint32_t v_s,
                                                       uint32_t lane, bool serial, int* lds_k, uint32_t* lds_s, uint32_t& c_skip,
                                                       uint32_t& c_ext, uint32_t& c_est, int& dk_bits, const bool lazy, int& amb_min
#if RBQ_STAMPS == 4
                                                       , unsigned long long* mst
#define MSTAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); mst[i] += t_ - mst[3]; mst[3] = t_; } while (0)
#else
#define MSTAMP(i)
#endif
                                                       ) {
#if RBQ_STAMPS == 4
        mst[3] = __builtin_amdgcn_s_memtime();
#endif
        const uint32_t len = HeapOps::uni(h.len);
        const bool taken = (mt >> lane) & 1ull;
        const bool fin = taken && ((v_d & 0x7f800000) != 0x7f800000);
        const int x = fin ? HeapOps::key(v_d) : kHigh;
        const unsigned long long finm = __ballot(fin);
        const bool odd = fin && !(__int_as_float(v_lb) < __int_as_float(v_d)); // lower bound not below the refined distance
        const unsigned long long oddm = __ballot(odd);
        // ---- one pass over the finite candidates i (s = its key): Q = #{candidates > own key} for run entries and
        //      candidates; the same compare, counted over the wave, is #{run entries < s} for lane i (empty lanes hold
        //      kHigh: never below s)
        int Q[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) Q[r] = 0;
        int QA = 0;
        uint32_t cB = 0;
        for (unsigned long long todo = finm; todo; todo &= todo - 1ull) {
            const uint32_t i = (uint32_t)__builtin_ctzll(todo);
            const int s = __builtin_amdgcn_readlane(x, (int)i);
            uint32_t cnt = 0;
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const int kr = r == 0 ? h.hd : h.xd[r];
                const bool gt = lazy ? s >= kr : s > kr; // (lazy: a candidate sits ABOVE the run entries of its key; empty lanes hold kHigh)
                Q[r] += gt ? 1 : 0;
                cnt += (uint32_t)__popcll(__ballot(gt));
            }
            QA += (s > x || (lazy && s == x && i > lane)) ? 1 : 0; // (lazy: equal candidates in lane order)
            cB = lane == i ? cnt : cB;
        }
        MSTAMP(0);
        bool tie = false;
        unsigned long long accm = finm; // candidates merged
        const uint32_t nfin = (uint32_t)__popcll(finm);
        if (!serial && oddm && len + nfin > top_k) {
            // the proviso: odd candidates that stay must have lb < t_end' = the element with exactly E elements above it
            const int E = (int)(len + nfin - top_k);
            int tkey = kHigh;
            bool found = false;
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t idx = (uint32_t)r * 64u + lane;
                const unsigned long long mm = __ballot(idx < len && (int)len - 1 - (int)idx + Q[r] == E);
                if (mm) { tkey = __builtin_amdgcn_readlane(r == 0 ? h.hd : h.xd[r], __builtin_ctzll(mm)); found = true; }
            }
            {
                const unsigned long long mm = __ballot(fin && (int)len - (int)cB + QA == E);
                if (mm) { tkey = __builtin_amdgcn_readlane(x, __builtin_ctzll(mm)); found = true; }
            }
            const float tf = __int_as_float(HeapOps::key(tkey));
            serial = !found || __ballot(odd && (int)len - (int)cB + QA >= E && !(__int_as_float(v_lb) < tf)) != 0ull;
        }
        if (serial) { // the reference's loop itself, on the run's top entries and the accepted candidates still alive
            uint32_t p = 0, size = len; // p: run entries that left (from the top)
            unsigned long long alive = 0ull;
            accm = 0ull;
            for (unsigned long long todo = mt; todo; todo &= todo - 1ull) {
                const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                const bool full = size == top_k;
                int tk = kHigh, bt = kLow, am = kLow;
                if (full) {
                    bt = p < len ? h.d_at(len - 1u - p) : kLow;
                    am = wave_max(((alive >> lane) & 1ull) ? x : kLow);
                    tk = bt > am ? bt : am;
                }
                const float tf = full ? __int_as_float(HeapOps::key(tk)) : INFINITY;
                const float lb = __int_as_float(__builtin_amdgcn_readlane(v_lb, (int)j));
                if (!(lb < tf)) { ++c_skip; continue; }
                ++c_ext;
                if (!((finm >> j) & 1ull)) continue;
                ++c_est;
                const int ke = __builtin_amdgcn_readlane(x, (int)j);
                if (full) {
                    if (ke > tk) continue;
                    if (ke == tk) { // turned away with the key of the maximum: which of the two the reference keeps depends on its heap
                        if (lazy) amb_min = amb_min < tk ? amb_min : tk; else tie = true;
                        continue;
                    }
                    if (bt >= am) ++p;
                    else alive &= ~(1ull << (uint32_t)__builtin_ctzll(__ballot(((alive >> lane) & 1ull) && x == am)));
                } else ++size;
                alive |= 1ull << j;
                accm |= 1ull << j;
            }
            // a candidate skipped by its lower bound may be smaller than elements that stay: count the accepted only
#pragma unroll
            for (int r = 0; r < TR; ++r) Q[r] = 0;
            QA = 0;
            for (unsigned long long todo = accm; todo; todo &= todo - 1ull) {
                const uint32_t i = (uint32_t)__builtin_ctzll(todo);
                const int s = __builtin_amdgcn_readlane(x, (int)i);
#pragma unroll
                for (int r = 0; r < TR; ++r) {
                    const int kr = r == 0 ? h.hd : h.xd[r];
                    Q[r] += (lazy ? s >= kr : s > kr) ? 1 : 0;
                }
                QA += (s > x || (lazy && s == x && i > lane)) ? 1 : 0;
            }
        }
        MSTAMP(1);
        // ---- merge: an element stays iff G = #{elements of run + merged candidates above it} >= E
        const uint32_t macc = (uint32_t)__popcll(accm);
        if (macc) {
            const uint32_t total = len + macc;
            const uint32_t evict = total > top_k ? total - top_k : 0u, nlen = total - evict;
#pragma unroll
            for (int r = 0; r < TR; ++r)
                if ((uint32_t)r * 64u + lane < nlen) lds_k[r * 64 + lane] = kHigh;
            int G[TR];
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t idx = (uint32_t)r * 64u + lane;
                G[r] = idx < len ? (int)len - 1 - (int)idx + Q[r] : -1;
                if (G[r] >= (int)evict) {
                    const uint32_t pos = nlen - 1u - (uint32_t)(G[r] - (int)evict);
                    lds_k[pos] = r == 0 ? h.hd : h.xd[r];
                    lds_s[pos] = r == 0 ? h.hs : h.xs[r];
                }
            }
            // (a run entry equal to x counts as above it: the pair lands side by side)
            const int GA = ((accm >> lane) & 1ull) ? (int)len - (int)cB + QA : -1;
            if (GA >= (int)evict) {
                const uint32_t pos = nlen - 1u - (uint32_t)(GA - (int)evict);
                lds_k[pos] = x;
                lds_s[pos] = v_s;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (evict) {
                // an element that leaves with the key of the new maximum: which of the two the reference keeps depends on
                // the layout of its heap
                const int newmax = lds_k[nlen - 1u];
                bool twin = GA >= 0 && GA < (int)evict && x == newmax;
#pragma unroll
                for (int r = 0; r < TR; ++r) twin |= G[r] >= 0 && G[r] < (int)evict && (r == 0 ? h.hd : h.xd[r]) == newmax;
                if (__ballot(twin) != 0ull) {
                    if (lazy) amb_min = amb_min < newmax ? amb_min : newmax; else tie = true;
                }
            }
            bool bad = false; // an unwritten position, or a key not above its lower neighbour
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t idx = (uint32_t)r * 64u + lane;
                const int kv = idx < nlen ? lds_k[idx] : kHigh;
                const uint32_t sv = idx < nlen ? lds_s[idx] : 0u;
                int below = __builtin_amdgcn_update_dpp(kLow, kv, 0x138, 0xf, 0xf, false); // wave_shr:1
                if (r > 0) {
                    const int carry = __builtin_amdgcn_readlane(r == 1 ? h.hd : h.xd[r - 1], 63);
                    below = lane == 0 ? carry : below;
                }
                bad |= idx < nlen && (kv == kHigh || (lazy ? below > kv : !(below < kv))); // (lazy: equal neighbours are in order)
                if (r == 0) { h.hd = kv; h.hs = sv; } else { h.xd[r] = kv; h.xs[r] = sv; }
            }
            tie |= __ballot(bad) != 0ull;
            h.len = nlen;
            if (nlen == top_k) dk_bits = HeapOps::key(h.d_at(top_k - 1u));
        }
        MSTAMP(2);
        return tie;
    }
};

// One register per lane (top_k <= 64): a SORTED RUN, entry i in lane i — one ballot pair and one DPP shift per
// insertion, the k-th distance is a readlane.  (With several registers the bag above is cheaper.)
template <int TR>
struct SortedRun {
    typedef int VI __attribute__((ext_vector_type(TR)));
    typedef uint32_t VU __attribute__((ext_vector_type(TR)));
    // k-th smallest distance (bits) of a run of `len` entries, +inf while the run is not full
    static __device__ __forceinline__ int kth(int d0, const VI& xd, uint32_t len, uint32_t top_k) {
        if (len < top_k) return 0x7f800000;
        const uint32_t kr = (top_k - 1u) >> 6;
        int v = d0;
#pragma unroll
        for (int r = 1; r < TR; ++r) v = kr == (uint32_t)r ? xd[r] : v; // kernel-uniform
        return __builtin_amdgcn_readlane(v, (int)HeapOps::uni((top_k - 1u) & 63u));
    }
    // insert (dbits, slot) into the run of `len` entries; returns true if an equal key was met
    static __device__ __forceinline__ bool insert(int& d0, uint32_t& s0, VI& xd, VU& xs, uint32_t len, int dbits, uint32_t slot,
                                                  uint32_t lane) {
        const int ke = HeapOps::key(dbits);
        uint32_t ipos = 0;
        bool tie = false;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (TR == 1 || (uint32_t)r * 64u < len) { // uniform: registers above the run hold nothing
                const int k = HeapOps::key(r == 0 ? d0 : xd[r]);
                const bool in = (uint32_t)r * 64u + lane < len;
                tie |= __ballot(in && k == ke) != 0ull;
                ipos += (uint32_t)__popcll(__ballot(in && k < ke)); // sorted: the smaller keys are a prefix
            }
        }
        const uint32_t rp = ipos >> 6, lp = ipos & 63u;
        // carries first (register r-1's OLD lane 63 enters register r at lane 0), then every register shifts
        VI cd = xd;
        VU cs = xs;
#pragma unroll
        for (int r = 1; r < TR; ++r) {
            cd[r] = __builtin_amdgcn_readlane(r == 1 ? d0 : xd[r - 1], 63);
            cs[r] = (uint32_t)__builtin_amdgcn_readlane((int)(r == 1 ? s0 : xs[r - 1]), 63);
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const int od = r == 0 ? d0 : xd[r];
            const uint32_t os = r == 0 ? s0 : xs[r];
            const int sd = __builtin_amdgcn_update_dpp(0, od, 0x138, 0xf, 0xf, false);      // wave_shr:1
            const int ss = __builtin_amdgcn_update_dpp(0, (int)os, 0x138, 0xf, 0xf, false);
            int nd = od;
            uint32_t ns = os;
            if (r > 0 && (uint32_t)r > rp) { // uniform
                nd = lane == 0 ? cd[r] : sd;
                ns = lane == 0 ? cs[r] : (uint32_t)ss;
            } else if ((uint32_t)r == rp) {
                nd = lane == lp ? dbits : (lane > lp ? sd : od);
                ns = lane == lp ? slot : (lane > lp ? (uint32_t)ss : os);
            }
            if (r == 0) { d0 = nd; s0 = ns; } else { xd[r] = nd; xs[r] = ns; }
        }
        return tie;
    }
};

// ---- the same BinaryHeap with LANE-PARALLEL primitives -------------------------------------------------------------------------
// RegHeap walks a sift level by level through v_readlane / compare-and-select (every hop a VALU -> SGPR -> VALU round trip:
// ~2-3 k cycles per push + pop at top_k = 100).  ParHeap holds the same array (entry g in lane g % 64 of register g / 64, raw
// distance bits) and gets the same result — Rust's std BinaryHeap, operation for operation — from what the operations DO to the array:
//   push(x)  sift_up moves x up its fixed ancestor chain while x > parent: the ancestors with key < x (a bottom prefix of the chain,
//            by the heap property) each move to their path child, x takes the topmost one's place.  One parallel step: every slot on
//            the chain looks at its parent.
//   pop()    the last element e replaces the root, sift_down_to_bottom takes the larger child at every level (`<=`: the right one on
//            equal keys) down to a leaf, sift_up brings e back up while e > parent.  Net effect: along that larger-child path the
//            nodes p_1 .. p_m with key >= e (a top prefix: keys fall along the path) move up one level, e lands in p_m's place, and
//            everything below is put back where it was.  So: every slot computes its larger child in parallel (children fetched with
//            ds_bpermute), a short scalar chain follows the path while key >= e, one parallel step applies it.
// ~4x fewer cycles per real heap operation; used by the tie log's replay (own function, own register allocation).
template <int TR>
struct ParHeap {
    int kd[TR];      // KEY (HeapOps::key of the distance bits: plain signed compares; its own inverse) of entry 64 r + lane
    uint32_t ks[TR]; // slots
    uint32_t len;    // uniform
    static constexpr uint32_t kNone = 0xffffffffu;
    static __device__ __forceinline__ int key(int b) { return HeapOps::key(b); }
    // value of entry idx (per lane; idx < 64 TR) of an array held in TR registers; S0..S1: the source registers idx can lie in
    template <typename T>
    __device__ __forceinline__ T fetch(const T (&a)[TR], uint32_t idx, int s0, int s1) const {
        T v = a[0];
        const int addr = (int)((idx & 63u) << 2);
#pragma unroll
        for (int s = 0; s < TR; ++s)
            if (s >= s0 && s <= s1) {
                const T t = (T)__builtin_amdgcn_ds_bpermute(addr, (int)a[s]);
                v = (idx >> 6) == (uint32_t)s ? t : v;
            }
        return v;
    }
    template <typename T>
    __device__ __forceinline__ T at(const T (&a)[TR], uint32_t i) const { // uniform index
        const uint32_t r = HeapOps::uni(i >> 6);
        T v = a[0];
#pragma unroll
        for (int k = 1; k < TR; ++k) v = r == (uint32_t)k ? a[k] : v;
        return (T)__builtin_amdgcn_readlane((int)v, (int)HeapOps::uni(i & 63u));
    }
    // is g a proper ancestor of slot n in the implicit tree?
    static __device__ __forceinline__ bool is_anc(uint32_t g, uint32_t n) {
        const int t = (int)__builtin_clz(g + 1u) - (int)__builtin_clz(n + 1u);
        return g < n && t > 0 && ((n + 1u) >> t) == g + 1u;
    }
    __device__ __forceinline__ void push(int kx, uint32_t xs, uint32_t lane) { // kx: the KEY of the new distance
        const uint32_t n = HeapOps::uni(len);
        int nk[TR];
        uint32_t ns[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const uint32_t g = (uint32_t)r * 64u + lane;
            const bool on_path = g == n || is_anc(g, n);
            const uint32_t par = g ? (g - 1u) >> 1 : 0u; // (lies in register <= r)
            const int pk = fetch(kd, par, (64 * r) / 128 > 0 ? (64 * r - 1) / 128 : 0, (64 * r + 62) / 128);
            const uint32_t ps = fetch(ks, par, (64 * r) / 128 > 0 ? (64 * r - 1) / 128 : 0, (64 * r + 62) / 128);
            const bool parent_moved = on_path && g > 0u && pk < kx;                 // the parent is an ancestor that x passes
            const bool takes_x = on_path && !parent_moved && (g == n || kd[r] < kx); // the top of the moved chain (or the slot itself)
            nk[r] = parent_moved ? pk : (takes_x ? kx : kd[r]);
            ns[r] = parent_moved ? ps : (takes_x ? xs : ks[r]);
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) { kd[r] = nk[r]; ks[r] = ns[r]; }
        len = n + 1u;
    }
    __device__ __forceinline__ void pop(uint32_t lane) {
        const uint32_t n = HeapOps::uni(len) - 1u; // the last element's index = the new length
        len = n;
        if (n == 0u) return;
        const int ke = at(kd, n);
        const uint32_t es = at(ks, n);
        // every slot's larger child — if that child stays above e (`e <= parent` ends the closing sift_up), else none: the scalar
        // chain below then needs ONE readlane per level
        uint32_t big[TR];
        int bk[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            big[r] = kNone; bk[r] = 0;
            if (128 * r + 1 < 64 * TR) { // (slots of this register can have children inside the array)
                const uint32_t g = (uint32_t)r * 64u + lane, cl = 2u * g + 1u, cr = 2u * g + 2u;
                const int s0 = 2 * r, s1 = 2 * r + 2 < TR ? 2 * r + 2 : TR - 1;
                const int kl = fetch(kd, cl & (64u * TR - 1u), s0, s1), kr = fetch(kd, cr & (64u * TR - 1u), s0, s1);
                const bool hasl = cl < n, right = cr < n && kl <= kr; // `hole.get(child) <= hole.get(child + 1)`: the right one
                bk[r] = right ? kr : kl;
                big[r] = (hasl && bk[r] >= ke) ? (right ? cr : cl) : kNone;
            }
        }
        unsigned long long take[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) take[r] = 0ull;
        uint32_t p = 0;
        for (;;) { // the larger-child path from the root while its nodes stay above e
            const uint32_t c = at(big, p);
            if (c == kNone) break;
#pragma unroll
            for (int r = 0; r < TR; ++r) if ((p >> 6) == (uint32_t)r) take[r] |= 1ull << (p & 63u);
            p = c;
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const bool tk = (take[r] >> lane) & 1ull, isp = (uint32_t)r * 64u + lane == p;
            uint32_t bs = 0u;
            if (128 * r + 1 < 64 * TR) bs = fetch(ks, big[r] & (64u * TR - 1u), 2 * r, 2 * r + 2 < TR ? 2 * r + 2 : TR - 1); // (the slot moves with the key)
            kd[r] = tk ? bk[r] : (isp ? ke : kd[r]);
            ks[r] = tk ? bs : (isp ? es : ks[r]);
        }
    }
    // some node of the root-to-slot-K path equals its off-path child (heap full: len == K)
    __device__ __forceinline__ bool path_tie(uint32_t K, uint32_t lane) const {
        bool t = false;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (128 * r + 1 < 64 * TR) {
                const uint32_t g = (uint32_t)r * 64u + lane, cl = 2u * g + 1u, cr = 2u * g + 2u;
                const int s0 = 2 * r, s1 = 2 * r + 2 < TR ? 2 * r + 2 : TR - 1;
                const int kl = fetch(kd, cl & (64u * TR - 1u), s0, s1), kr = fetch(kd, cr & (64u * TR - 1u), s0, s1);
                const bool anc = is_anc(g, K);
                const bool left_on_path = cl == K || is_anc(cl, K); // (else the right child is the path child)
                const uint32_t off = left_on_path ? cr : cl;
                t |= anc && off < K && kd[r] == (left_on_path ? kr : kl);
            }
        }
        return __ballot(t) != 0ull;
    }
};

// The reference's prune / push / pop loop (src/ivf.rs:2054-2126) over a query's logged candidates, with the BinaryHeap emulation: what a
// tied query runs instead of scanning its lists again (k_scan, `tie_log`).  One wave; the heap lives in registers (ParHeap) or, for
// top_k = 64 TR exactly, in LDS.  Returns the heap (everything by value: an argument passed by reference would pin the caller's top-k
// registers to memory for the whole kernel); `len` of the result is the heap's length in both cases.
template <int TR>
__device__ __attribute__((noinline)) RegHeap<TR> tie_log_replay(float* heap_d, uint32_t* heap_s, const uint32_t* tlog, uint32_t log_n,
                                                                uint32_t top_k, bool reg_heap, uint32_t lane, unsigned int* stats) {
    uint32_t n_real = 0;
#ifdef RBQ_TIE_TIMING
    const unsigned long long tt0 = __builtin_amdgcn_s_memtime();
#endif
    ParHeap<TR> ph;
#pragma unroll
    for (int r = 0; r < TR; ++r) { ph.kd[r] = 0; ph.ks[r] = 0u; }
    ph.len = 0u;
    LdsHeap lh{heap_d, heap_s, 0};
    // PUSH-THEN-POP IS THE IDENTITY.  Most evaluated candidates of a full heap lie above its root: the reference pushes them and pops
    // them again (src/ivf.rs:2116-2126).  With Rust's BinaryHeap (sift_up; pop = swap the last element into the root,
    // sift_down_to_bottom, sift_up) that pair leaves the array exactly as it was: the new key x > root climbs the path from slot k
    // to the root, shifting the path's elements down by one; pop removes the element now in slot k, puts it in the root, and the hole
    // walks back DOWN THE SAME PATH — at every path node the path child holds the node's own old value, which is >= the off-path
    // child — restoring every element, and the displaced one ends where it came from.  The only way off the path is a comparison
    // of EQUAL keys (`<=` picks the right child; the closing sift_up stops at `<=`), i.e. a path node whose old value equals its
    // off-path child's.  `ptie` = some node of the (fixed: top_k is) root-to-slot-k path equals its off-path child (conservative);
    // while it is false a candidate with key > root key is skipped in O(1); it is re-evaluated (lazily) after a real insertion.
    bool ptie = false, ptie_valid = true;
    auto lds_path_tie = [&]() -> bool {
        bool t = false;
        for (uint32_t c = top_k; c > 0;) {
            const uint32_t par = (c - 1u) >> 1, sib = (c & 1u) ? c + 1u : c - 1u;
            if (sib < top_k) t |= __float_as_int(heap_d[par]) == __float_as_int(heap_d[sib]);
            c = par;
        }
        return t;
    };
    for (uint32_t c0 = 0; c0 < log_n; c0 += 64u) {
        const uint32_t cn = log_n - c0 < 64u ? log_n - c0 : 64u;
        int e_lb = 0, e_d = 0;
        uint32_t e_s = 0;
        if (lane < cn) { const uint32_t* e = tlog + (size_t)(c0 + lane) * 3u; e_lb = (int)e[0]; e_d = (int)e[1]; e_s = e[2]; }
        for (uint32_t j = 0; j < cn; ++j) {
            const float lb = __int_as_float(__builtin_amdgcn_readlane(e_lb, (int)j));
            const int dbits = __builtin_amdgcn_readlane(e_d, (int)j);
            const uint32_t hlen = reg_heap ? HeapOps::uni(ph.len) : lh.len;
            const bool full = hlen == top_k;
            const int rootb = !full ? 0x7f800000 : (reg_heap ? HeapOps::key(__builtin_amdgcn_readlane(ph.kd[0], 0)) : __float_as_int(heap_d[0]));
            if (lb >= __int_as_float(rootb)) continue;                  // `lower_bound >= distk`: skipped
            if (!finite_f(__int_as_float(dbits))) continue;             // non-finite distance: dropped
            if (full && HeapOps::key(dbits) > HeapOps::key(rootb)) {    // pushed and popped again: the heap is unchanged ...
                if (!ptie_valid) { ptie = reg_heap ? ph.path_tie(top_k, lane) : lds_path_tie(); ptie_valid = true; }
                if (!ptie) continue;                                    // ... unless equal keys sit on the path
            }
            const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)e_s, (int)j);
            ++n_real;
            if (reg_heap) {
                ph.push(HeapOps::key(dbits), slot, lane);
                if (ph.len > top_k) ph.pop(lane);
            } else {
                if (lane == 0) {
                    lh.push(__int_as_float(dbits), slot);
                    if (lh.len > top_k) lh.pop();
                }
                lh.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)lh.len);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            ptie_valid = false;
        }
    }
    if (stats && lane == 0) { atomicAdd(stats, 1u); atomicAdd(stats + 1, log_n); atomicAdd(stats + 2, n_real); }
#ifdef RBQ_TIE_TIMING
    if (stats && lane == 0) atomicAdd(stats + 3, (unsigned int)((__builtin_amdgcn_s_memtime() - tt0) >> 6)); // (diagnostic build: slot 3 = ticks / 64)
#endif
    RegHeap<TR> rh;
    rh.hd = HeapOps::key(ph.kd[0]); rh.hs = ph.ks[0]; rh.xd = 0; rh.xs = 0u; // (keys back to distance bits)
#pragma unroll
    for (int r = 1; r < TR; ++r) { rh.xd[r] = HeapOps::key(ph.kd[r]); rh.xs[r] = ph.ks[r]; }
    rh.len = reg_heap ? ph.len : lh.len;
    return rh;
}

#ifndef RBQ_REPLAY_PRIO
#define RBQ_REPLAY_PRIO 3
#endif
#ifndef RBQ_SCAN_LAZY_TIES
#define RBQ_SCAN_LAZY_TIES 1  // k_scan settles equal distances by the lazy-tie rule (0: any equal pair re-runs the query, rounds 2-4)
#endif
#ifndef RBQ_HEAVY_PER
#define RBQ_HEAVY_PER 1
#endif
#ifndef RBQ_WIN_GROW
#define RBQ_WIN_GROW 4
#endif
#ifndef RBQ_WIN0
#define RBQ_WIN0 kTB // stream entries examined by the first fill step (one tile's worth)
#endif
// EX: compile-time ex_bits (0/2/6) when DT != 0; ignored (runtime P.ex_bits) when DT == 0.
// TR: registers per lane of the replay wave's top-k (1: top_k <= 63; 2: <= 128; 4: <= 256 — with more than one,
// four waves per SIMD instead of five).
// V: numeric variant (kernels.hpp, kVarAvx512 / kVarAvx2 / kVarPortable).  The variants other than the default are instantiated
// for the runtime-dimension kernel only (DT = 0), so the default instantiations keep their code and the build its size.
template <int DT, int EX, int TR, int V = kVarAvx512>
__global__ __launch_bounds__(kScanThreads, ((TR == 1 && scan_nb((uint32_t)DT) == 1) ? RBQ_SCAN_WAVES : 4)) void k_scan(ScanParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    // blocks per scanner half-wave and tile: 1; a build option gives 2 at small dimensions (types.hpp: measured, not faster)
    constexpr int NB = scan_nb((uint32_t)DT);
    constexpr int kTB = kTileBlocks * NB;  // blocks per tile
    constexpr int kTC = kTileCand * NB;    // candidates per tile
    const uint32_t Dc = DT ? (uint32_t)DT : P.Dc; // code/LUT dimension (x64)
    const uint32_t D = DT ? (uint32_t)DT : P.D;   // padded_dim (ex codes, rotated query)
    uint8_t* s_lut = smraw;
    float* s_q = reinterpret_cast<float*>(smraw + (size_t)Dc * 4);
    // the exact heap of top_k + 1 entries: in LDS, or (top_k beyond the LDS: the reference accepts any top_k, src/ivf.rs:2116-2126)
    // in this query's slice of a global workspace — one lane works on it either way
    const uint32_t hk = P.heap_ws ? 0u : P.top_k + 1u;
    float* heap_d = s_q + ex_qlen(D, DT ? (uint32_t)EX : P.ex_bits);
    uint32_t* heap_s = reinterpret_cast<uint32_t*>(heap_d + hk);
    uint32_t* q_slot = heap_s + hk;                      // [2][kTileCand]
    if (P.heap_ws) {
        heap_d = reinterpret_cast<float*>(P.heap_ws + (size_t)blockIdx.x * 2 * ((size_t)P.top_k + 1));
        heap_s = reinterpret_cast<uint32_t*>(heap_d + (P.top_k + 1));
    }
    float* q_lb = reinterpret_cast<float*>(q_slot + 2 * kTC);
    float* q_ip = q_lb + 2 * kTC;
    float* q_gadd = q_ip + 2 * kTC;
    float* q_d = q_gadd + 2 * kTC;
    uint32_t* s_list = reinterpret_cast<uint32_t*>(q_d + 2 * kTC); // [kTC] survivor positions, stream order
    uint32_t* s_mask = s_list + kTC;                                // [2][kTB]
    WorkItem* s_queue = reinterpret_cast<WorkItem*>(s_mask + 2 * kTB); // [kQueueCap] live blocks, stream order
    unsigned long long* s_fmask = reinterpret_cast<unsigned long long*>(s_queue + kQueueCap); // [kFillK][kNScan] fill-step live masks
    // no static __shared__ in this kernel: the dynamic region must start at LDS address 0 (see lds_lut_ptr)
    uint32_t* s_misc = reinterpret_cast<uint32_t*>(s_fmask + kNScan * kFillK);
    float& s_T = *reinterpret_cast<float*>(s_misc);
    uint32_t& s_len = *(s_misc + 1);
    uint32_t* s_nskip = s_misc + 2;
    uint32_t& s_nbatch = *(s_misc + 3);   // refine batch size of the current round (kBatchDone = tile finished)
    uint32_t& s_restart = *(s_misc + 4);  // a distance tie was met on the sorted fast path: re-run with the exact heap
    uint32_t* s_batch = s_misc + 8;       // [2*kScanThreads/16] queue positions to refine in this round

    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t wave = tid >> 6, lane = tid & 63u, half = lane >> 5, l32 = lane & 31u;
    const uint32_t hw = tid >> 5; // half-wave index; scanners own blocks 0..kTileBlocks-1 of a tile
    const bool scanner = wave < (uint32_t)kNScan;
    const lds_lut_ptr lut0 = (lds_lut_ptr)(uint32_t)0; // == s_lut
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smraw != 0u) __builtin_trap();
    const uint32_t top_k = P.top_k;
    const uint32_t ex_bits = DT ? (uint32_t)EX : P.ex_bits;
    const size_t stride = (size_t)Dc * 4 + 384;
    const size_t exb = ex_bytes_dev(D, ex_bits);
    const uint32_t nunits = ex_w4(D, ex_bits), qlen = ex_qlen(D, ex_bits);

    {
        const uint4* src = reinterpret_cast<const uint4*>(P.lut + (size_t)q * Dc * 4);
        uint4* dst = reinterpret_cast<uint4*>(s_lut);
        for (uint32_t i = tid; i < Dc / 4; i += kScanThreads) dst[i] = src[i];
        // (the rotated query as 16-byte loads, all of a thread's in flight before its first LDS store: the plain dword loop waited for
        // every load in front of its ds_write — four dependent round trips at D = 960 before the first fill step)
        const float4* rs = reinterpret_cast<const float4*>(P.rot + (size_t)q * D); // (D % 4 == 0: padded_dim is a multiple of 64)
        float4* rd = reinterpret_cast<float4*>(s_q);
        for (uint32_t i0 = tid; i0 < qlen / 4; i0 += 2 * kScanThreads) {
            float4 b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) { const uint32_t i = i0 + (uint32_t)u * kScanThreads; b[u] = (i < qlen / 4 && i < D / 4) ? rs[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
#pragma unroll
            for (int u = 0; u < 2; ++u) { const uint32_t i = i0 + (uint32_t)u * kScanThreads; if (i < qlen / 4) rd[i] = b[u]; }
        }
        if (tid == 0) { s_T = INFINITY; *s_nskip = 0; s_len = 0; s_restart = 0; s_misc[5] = 0; s_misc[6] = 0; s_misc[7] = 0; }
    }
    // the replay wave is the serial part of every tile: let it issue ahead of the (many) scanner waves it shares
    // its SIMD with
    if (!scanner) __builtin_amdgcn_s_setprio(RBQ_REPLAY_PRIO);
    const QueryConsts qc = P.consts[q];
    const ProbeInfo* probe = P.probe + (size_t)q * P.nprobe;
    const StreamItem* wl = P.wl + (size_t)q * P.wl_stride;
    const uint32_t ns = P.nstream[q];
    __syncthreads();

    uint32_t n_skip = 0, n_ext = 0, n_est = 0; // n_skip: every thread; n_ext/n_est: replay wave (uniform)
    // traffic counters of an open profile (P.prof): block records whose codes / factor rows this half-wave
    // requested, passes over the stream, ex-code evaluations (they survive an exact-heap restart: the traffic is real)
    uint32_t p_code = 0, p_meta = 0, p_pass = 1; // (candidates whose ex codes were fetched are counted in s_misc[7])
    const bool count_skips = P.diag != nullptr;

    bool fast = top_k <= 64u * TR && !P.exact_heap && !P.mstg; // sorted run (SortedRun / RankRun) until a distance tie shows up
    uint32_t* const tlog = P.tie_log ? P.tie_log + (size_t)q * P.tie_log_cap * 3u : nullptr; // tie log of this query (see `log_n` below)
    // group `g` (16 lanes) refines the survivor at queue position s_batch[g] of tile buffer `buf`.  The ex
    // factors are requested together with the code units, not after the dot product.
    auto refine_batch = [&](uint32_t buf, uint32_t nb, uint32_t g) {
        const uint32_t gl = tid & 15u;
        if (g < nb) {
            const uint32_t e = buf * kTC + s_batch[g];
            const uint32_t sl = q_slot[e];
            const uint8_t* ex = P.ex_codes + (size_t)sl * exb;
            float sacc;
            float fa, fr;
            if constexpr (V != kVarAvx512) {
                fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                sacc = ex_dot_var_rt<V>(ex, s_q, gl, nunits, D / 16, ex_bits); // (already the group's sum)
            } else if (nunits <= (uint32_t)kExRegUnits) {
                uint4 u[kExRegUnits];
                ex_load_all(u, ex, gl, nunits);
                fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                asm volatile("" : "+v"(fa), "+v"(fr)); // issue the loads here
                sacc = ex_bits == 6 ? ex_dot_all<6>(u, s_q, gl, nunits) : ex_dot_all<2>(u, s_q, gl, nunits);
            } else {
                fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                asm volatile("" : "+v"(fa), "+v"(fr));
                sacc = ex_bits == 6 ? ex_dot_units<6>(ex, s_q, gl, nunits) : ex_dot_units<2>(ex, s_q, gl, nunits);
            }
            if constexpr (V == kVarAvx512) sacc = group16_reduce(sacc);
            if (gl == 0) {
                float tt2 = qc.scale * q_ip[e];
                tt2 = tt2 + sacc;
                tt2 = tt2 + qc.kbx;
                const float a = fa + q_gadd[e];
                const float m = fr * tt2;
                q_d[e] = a + m;
            }
        }
    };

    // small dimensions (one code unit per lane): group `g` of `ng` refines the survivors at queue positions
    // s_batch[g] and s_batch[g + ng] in one pass
    // heavy tiles: survivors a 16-lane group refines per round when a vector's codes span several units (one after the
    // other; twice the batch = half the rounds of barrier + collect + replay, at the price of a larger superset)
    constexpr int kHeavyPer = RBQ_HEAVY_PER;
    constexpr uint32_t kNU = ex_w4((uint32_t)(DT ? DT : 16), (uint32_t)(EX ? EX : 2)); // code units per lane and vector
    constexpr bool kDual1 = DT != 0 && EX != 0 && kNU == 1u;
#ifndef RBQ_PAIR_UNITS
#define RBQ_PAIR_UNITS 1
#endif
    constexpr bool kDualN = RBQ_PAIR_UNITS && DT != 0 && EX != 0 && TR > 1 && kNU >= 2u && kNU <= 3u; // packed pair refine (top_k >= 64)
    constexpr bool kDual = kDual1 || kDualN;
    auto refine_pair = [&](uint32_t buf, uint32_t nb, uint32_t g, uint32_t ng) {
        const uint32_t gl = tid & 15u;
        if (g >= nb) return;
        const bool has1 = g + ng < nb;
        const uint32_t e0 = buf * kTC + s_batch[g];
        const uint32_t e1 = buf * kTC + s_batch[has1 ? g + ng : g];
        const uint32_t sl0 = q_slot[e0], sl1 = q_slot[e1];
        const uint4* p0 = reinterpret_cast<const uint4*>(P.ex_codes + (size_t)sl0 * exb) + gl;
        const uint4* p1 = reinterpret_cast<const uint4*>(P.ex_codes + (size_t)sl1 * exb) + gl;
        // (no register pin on the four factor loads: it made the wave WAIT for them before the code units were even requested)
        const float fa0 = P.f_add_ex[sl0], fr0 = P.f_rescale_ex[sl0], fa1 = P.f_add_ex[sl1], fr1 = P.f_rescale_ex[sl1];
        float sa, sb;
        if constexpr (V != kVarAvx512) { // (not reached: the variants are DT = 0 instantiations, which never pair)
            sa = ex_dot_var_rt<V>(P.ex_codes + (size_t)sl0 * exb, s_q, gl, nunits, D / 16, ex_bits);
            sb = ex_dot_var_rt<V>(P.ex_codes + (size_t)sl1 * exb, s_q, gl, nunits, D / 16, ex_bits);
        } else if (kDualN) ex_dot_pair_all<(EX ? EX : 2), (kDualN ? (int)kNU : 1)>(p0, p1, s_q, gl, sa, sb);
        else {
            const uint4 u0 = p0[0], u1 = p1[0];
            if (EX == 6) ex_dot_pair1<6>(u0, u1, s_q, gl, D / 16, sa, sb);
            else ex_dot_pair1<(EX ? EX : 2)>(u0, u1, s_q, gl, D / 16, sa, sb);
        }
        if constexpr (V == kVarAvx512) {
            sa = group16_reduce(sa);
            sb = group16_reduce(sb);
        }
        if (gl == 0) {
            {
                float tt2 = qc.scale * q_ip[e0];
                tt2 = tt2 + sa;
                tt2 = tt2 + qc.kbx;
                const float a = fa0 + q_gadd[e0];
                const float m = fr0 * tt2;
                q_d[e0] = a + m;
            }
            if (has1) {
                float tt2 = qc.scale * q_ip[e1];
                tt2 = tt2 + sb;
                tt2 = tt2 + qc.kbx;
                const float a = fa1 + q_gadd[e1];
                const float m = fr1 * tt2;
                q_d[e1] = a + m;
            }
        }
    };

    struct Meta { float f_add, f_rescale, f_error, g_add, g_err, dotqc; };
    auto load_meta = [&](const WorkItem& w) -> Meta {
        const float* fac = reinterpret_cast<const float*>(P.blocks + (size_t)w.gblock * stride + (size_t)Dc * 4);
        const ProbeInfo pi = probe[w.rank_nvalid >> 6];
        Meta m;
        m.f_add = fac[l32]; m.f_rescale = fac[32 + l32]; m.f_error = fac[64 + l32];
        m.g_add = pi.g_add; m.g_err = pi.g_err; m.dotqc = pi.dotqc;
        return m;
    };
    // lower bound of one candidate as a function of its accumulator value: the exact operation sequence of
    // the epilogue (compute_batch_distances_u16, AVX2 body: only the first op is fused; kVarPortable: the scalar body, not
    // fused at all), so floating-point monotonicity carries over to the bound below
    auto lb_of = [&](const Meta& m, float accu_f, float& ip, float& est) -> float {
        ip = epi_ip(qc.delta, accu_f, qc.sum_vl, V == kVarPortable);
        const float tt = ip + qc.k1x;
        const float rs = m.f_rescale * tt;
        est = m.f_add + m.g_add;
        est = est + rs;
        const float er = m.f_error * m.g_err;
        return est - er;
    };
    // Block-level bound: accu of any code lies in [amin, amax] and lb is monotone in accu (direction = sign
    // of f_rescale), so min(lb(amin), lb(amax)) <= lb(true accu).  If that already reaches the (stale, hence
    // larger) threshold for every lane, the reference skips all of these candidates too and the block's
    // codes are never read.  Disabled when accu could wrap (amax > 65535) and when filtered diagnostics need
    // per-candidate filter tests.
    const bool bound_ok = qc.amax <= 65535.0f && !(P.filter && P.diag) && !P.no_block_bound;
    auto lane_prunable = [&](const WorkItem& w, const Meta& m, float T) -> bool {
        float d0, d1;
        const float a = lb_of(m, qc.amin, d0, d1), b = lb_of(m, qc.amax, d0, d1);
        const bool prunable = finite_f(a) && finite_f(b) && fminf(a, b) >= T;
        return (l32 >= (w.rank_nvalid & 63u)) || prunable;
    };

    // Uniform loop state (identical in every wave; advanced only from LDS values published before a barrier)
    uint32_t pos = 0;                 // next unexamined stream block
    uint32_t qhead = 0, qcount = 0;   // live-block FIFO
    uint32_t tile = 0;                // tiles published so far (buffer = tile & 1)
    // Blocks examined by the next fill step.  The first steps are small: with the threshold still at +inf the
    // block bound passes everything, and whatever is queued then is paid for at tile time (factor rows, a
    // barrier, usually no survivor).  Once the nearest lists have set a threshold the windows grow
    // (x RBQ_WIN_GROW per step, up to kFillK entries per scanner lane).
    uint32_t win = (uint32_t)(RBQ_WIN0);
    // replay-wave state
    const bool reg_heap = top_k < 64u * TR;                     // exact BinaryHeap emulation in registers (else in LDS)
    // RankRun from top_k = 64; below, the one-register sorted run (RankRun there costs the hot kernel 20 bytes of scratch at
    // five waves per SIMD, and at top_k = 10 most candidates are rejected by one scalar compare anyway)
    constexpr bool kRank = TR > 1;
    RegHeap<TR> rh; // the replay wave's top-k registers: exact heap, or (same registers) the bag
    rh.hd = 0; rh.hs = 0u; rh.xd = 0; rh.xs = 0u; rh.len = 0u;
    if (kRank && fast) RankRun<TR>::clear(rh); // keys, empty lanes marked
    int bag_dk = 0x7f800000; // RankRun: bits of the k-th distance (valid once the run holds top_k entries)
    bool tie_pending = false; // replay wave: a distance tie was met, the query will be re-run with the exact heap
    // LAZY TIES (round 5, as in k_scanw — the rule and its proof are at `amb_min` in scanw.hpp): equal distances do not end the fast
    // pass; the smallest key with which an element left (or was turned away) while its twin stayed is recorded, and the final run
    // decides at the end of the stream whether the reference's result depends on the layout of its heap.
    constexpr bool kLazyTies = RBQ_SCAN_LAZY_TIES != 0;
    int amb_min = 0x7fffffff;
    // TIE LOG: every candidate a refine batch takes (a superset, in stream order, of the ones the reference evaluates) is written to
    // the query's log with its lower bound, refined distance and slot.  The reference's own loop over exactly these candidates —
    // `lower_bound >= distk` -> skip, push, pop — is a function of that sequence alone (a candidate outside the log has
    // lb >= a threshold that was already >= the reference's: skipped there too), so a tied query replays the log through the exact
    // heap instead of scanning its lists again.
    uint32_t log_n = 0; // replay wave, uniform: entries logged so far (may pass the capacity: then the log is not used)
    LdsHeap lh{heap_d, heap_s, 0};
#ifdef RBQ_STAMPS
    unsigned long long st_total = __builtin_amdgcn_s_memtime(), st_heavy = 0, st_waitA = 0, st_look = 0, st_fill = 0, st_a, st_b, st_c;
    uint32_t st_nheavy = 0, st_surv = 0, st_ntile = 0, st_dead = 0;
    uint32_t st_rounds = 0;
#define STAMP(x) x = __builtin_amdgcn_s_memtime()
    unsigned long long rp_collect = 0, rp_ref0 = 0, rp_replay = 0, rp_waitC = 0, rp_light = 0, rp_waitA = 0, r0 = 0, r1 = 0, rp_x1 = 0, rp_x2 = 0;
    unsigned long long mst[4] = {0, 0, 0, 0}; // RankRun::merge_batch phases (RBQ_STAMPS == 4)
#define RSTAMP(acc) do { r1 = __builtin_amdgcn_s_memtime(); acc += r1 - r0; r0 = r1; } while (0)
#else
#define STAMP(x)
#define RSTAMP(acc)
#endif

#ifdef RBQ_STAMPS
    const unsigned long long st_loop0 = __builtin_amdgcn_s_memtime();
    unsigned long long st_tiles = 0, st_t0 = 0;
#endif
  for (;;) { // a second pass only after a tie on the sorted fast path
    while (true) {
        if (pos < ns && qcount < (uint32_t)kTB) {
            // ---------------------------------------------------------------- fill step: examine `win` stream entries
            STAMP(st_c);
            if (scanner) {
                // kFillK stream entries per lane (entry k*192 + lane slot of the window): precomputed block-level
                // bound vs the threshold; compaction in stream order = (k, wave, lane) order
                const float T = s_T;
                const uint32_t wslot = wave * 64u + lane;
                WorkItem w[kFillK];
                bool live[kFillK];
                StreamItem si[kFillK];
#pragma unroll
                for (int k = 0; k < kFillK; ++k) {
                    const uint32_t wk = (uint32_t)k * (kNScan * 64u) + wslot;
                    si[k].gblock = 0; si[k].rank_nvalid = 0; si[k].lbmin = 0.0f; si[k].pad = 0;
                    live[k] = wk < win && pos + wk < ns;
                    if (live[k]) si[k] = wl[pos + wk];
                }
                unsigned long long lm[kFillK];
#pragma unroll
                for (int k = 0; k < kFillK; ++k) {
                    w[k].gblock = si[k].gblock; w[k].rank_nvalid = si[k].rank_nvalid;
                    if (live[k] && bound_ok && si[k].lbmin >= T) { // block_lbmin(): no real vector of the block can pass
                        live[k] = false;
                        if (count_skips) n_skip += w[k].rank_nvalid & 63u;
                    }
                    lm[k] = __ballot(live[k]);
                    if (lane == 0) s_fmask[k * kNScan + wave] = lm[k];
                }
                lds_barrier(); // X1: live masks published
                uint32_t total = 0;
#pragma unroll
                for (int j = 0; j < kNScan * kFillK; ++j) total += __popcll(s_fmask[j]);
                {
                    uint32_t base = 0; // running count of the sub-windows before k
#pragma unroll
                    for (int k = 0; k < kFillK; ++k) {
                        uint32_t cnt_k = 0;
#pragma unroll
                        for (int j = 0; j < kNScan; ++j) cnt_k += __popcll(s_fmask[k * kNScan + j]);
                        uint32_t offk = 0;
#pragma unroll
                        for (int j = 0; j < kNScan; ++j) if ((uint32_t)j < wave) offk += __popcll(s_fmask[k * kNScan + j]);
                        if (live[k]) s_queue[(qhead + qcount + base + offk + __popcll(lm[k] & ((1ull << lane) - 1ull))) % kQueueCap] = w[k];
                        base += cnt_k;
                    }
                }
                lds_barrier(); // X2: queue entries visible
                qcount += total;
            } else {
                lds_barrier(); // X1
                uint32_t total = 0;
#pragma unroll
                for (int j = 0; j < kNScan * kFillK; ++j) total += __popcll(s_fmask[j]);
                lds_barrier(); // X2
                qcount += total;
            }
            pos += win;
            win = win * (uint32_t)RBQ_WIN_GROW < (uint32_t)kWindow ? win * (uint32_t)RBQ_WIN_GROW : (uint32_t)kWindow;
#ifdef RBQ_STAMPS
            STAMP(st_b); st_fill += st_b - st_c;
#endif
            continue;
        }
        if (qcount == 0) break;
        // -------------------------------------------------------------------- tile step
        STAMP(st_t0);
        const uint32_t n = qcount < (uint32_t)kTB ? qcount : (uint32_t)kTB;
        const uint32_t buf = tile & 1u;
        if (scanner) {
          if constexpr (NB == 1) { // one block per half-wave and tile
            WorkItem wi_c;
            wi_c.gblock = 0; wi_c.rank_nvalid = 0;
            if (hw < n) wi_c = s_queue[(qhead + hw) % kQueueCap];
            const uint8_t* blk = P.blocks + (size_t)wi_c.gblock * stride;
            // The codes are requested together with the factor rows, not after the bound below: a queued block
            // already passed the block-level bound of the fill step, so it is almost always still alive, and the
            // two memory round trips overlap (the runtime-dimension path keeps the lazy order).
            CodeRegs<DT> cc;
            if (DT && hw < n) load_codes<DT>(cc, blk, l32);
            if (hw < n) { ++p_meta; if (DT) ++p_code; }
            const Meta m_c = load_meta(wi_c);
            const float T = s_T;
            // per-lane bound with the fresh threshold: the whole wave may be prunable without looking anything up
            const bool live_c = !bound_ok || (__ballot(lane_prunable(wi_c, m_c, T)) != ~0ull);
            const uint32_t nvalid = wi_c.rank_nvalid & 63u;
            const uint32_t slot = wi_c.gblock * 32u + l32;
            bool valid = l32 < nvalid;
            if (valid && P.filter) {
                const uint32_t id32 = (uint32_t)P.ids[slot];
                valid = ((uint64_t)id32 < P.filter_nbits) && ((P.filter[id32 >> 5] >> (id32 & 31u)) & 1u);
            }
            bool surv = false;
            float lb = 0.0f, ip = 0.0f, est = 0.0f;
#ifdef RBQ_STAMPS
            ++st_ntile; if (!live_c) ++st_dead;
#endif
            if (live_c) { // wave-uniform
                STAMP(st_a);
                if (!DT && hw < n) ++p_code;
                const uint32_t accu = (DT ? lookup_codes<DT>(cc, blk, l32, lut0) : accumulate_block_rt(blk, lut0, l32, Dc)) & 0xffffu;
#ifdef RBQ_STAMPS
                asm volatile("" :: "v"(accu));
                STAMP(st_b); st_look += st_b - st_a;
#endif
                lb = lb_of(m_c, (float)accu, ip, est);
                if (P.mstg) {
                    if (!finite_f(est)) valid = false;          // `if distance.is_finite()`
                    if (P.metric == 0) est = fmaxf(est, 0.0f);  // distance.max(0.0)
                    lb = est;                                   // f_error row and g_error are zero
                } else if (!finite_f(lb)) {
                    lb = P.metric == 0 ? 0.0f : -(m_c.dotqc + qc.qnorm);
                    // the reference skips iff `lower_bound >= distk` (src/ivf.rs:2054): a NaN bound (NaN query, inner product)
                    // is never skipped.  -inf decides every such test the same way and keeps `lb < T` usable below.
                    if (lb != lb) lb = -INFINITY;
                }
                surv = valid && (lb < T);
            }
            if (valid && !surv) ++n_skip;
            const unsigned long long bal = __ballot(surv);
            const uint32_t mask32 = (uint32_t)(bal >> (half * 32));
            if (l32 == 0) s_mask[buf * kTileBlocks + hw] = mask32;
            if (surv) {
                const uint32_t e = buf * kTileCand + hw * 32u + l32;
                q_slot[e] = slot;
                q_lb[e] = lb;
                q_ip[e] = ip;
                q_gadd[e] = m_c.g_add;
                q_d[e] = est;
            }
          } else {
            // half-wave hw scans blocks hw, hw + kTileBlocks, ... of the tile (NB of them); everything of all of them is requested
            // before the first lookup
            WorkItem wi_c[NB];
            const uint8_t* blk[NB];
            CodeRegs<DT> cc[NB];
            Meta m_c[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const uint32_t bi = hw + (uint32_t)(kTileBlocks * i);
                wi_c[i].gblock = 0; wi_c[i].rank_nvalid = 0;
                if (bi < n) wi_c[i] = s_queue[(qhead + bi) % kQueueCap];
                blk[i] = P.blocks + (size_t)wi_c[i].gblock * stride;
                // The codes are requested together with the factor rows, not after the bound below: a queued block
                // already passed the block-level bound of the fill step, so it is almost always still alive, and the
                // two memory round trips overlap (the runtime-dimension path keeps the lazy order).
                if (DT && bi < n) load_codes<DT>(cc[i], blk[i], l32);
                if (bi < n) { ++p_meta; if (DT) ++p_code; }
                m_c[i] = load_meta(wi_c[i]);
            }
            const float T = s_T;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const uint32_t bi = hw + (uint32_t)(kTileBlocks * i);
                // per-lane bound with the fresh threshold: the whole wave may be prunable without looking anything up
                const bool live_c = !bound_ok || (__ballot(lane_prunable(wi_c[i], m_c[i], T)) != ~0ull);
                const uint32_t nvalid = wi_c[i].rank_nvalid & 63u;
                const uint32_t slot = wi_c[i].gblock * 32u + l32;
                bool valid = l32 < nvalid;
                if (valid && P.filter) {
                    const uint32_t id32 = (uint32_t)P.ids[slot];
                    valid = ((uint64_t)id32 < P.filter_nbits) && ((P.filter[id32 >> 5] >> (id32 & 31u)) & 1u);
                }
                bool surv = false;
                float lb = 0.0f, ip = 0.0f, est = 0.0f;
#ifdef RBQ_STAMPS
                ++st_ntile; if (!live_c) ++st_dead;
#endif
                if (live_c) { // wave-uniform
                    STAMP(st_a);
                    if (!DT && bi < n) ++p_code;
                    const uint32_t accu = (DT ? lookup_codes<DT>(cc[i], blk[i], l32, lut0) : accumulate_block_rt(blk[i], lut0, l32, Dc)) & 0xffffu;
#ifdef RBQ_STAMPS
                    asm volatile("" :: "v"(accu));
                    STAMP(st_b); st_look += st_b - st_a;
#endif
                    lb = lb_of(m_c[i], (float)accu, ip, est);
                    if (P.mstg) {
                        if (!finite_f(est)) valid = false;          // `if distance.is_finite()`
                        if (P.metric == 0) est = fmaxf(est, 0.0f);  // distance.max(0.0)
                        lb = est;                                   // f_error row and g_error are zero
                    } else if (!finite_f(lb)) {
                        lb = P.metric == 0 ? 0.0f : -(m_c[i].dotqc + qc.qnorm);
                        if (lb != lb) lb = -INFINITY; // (NaN is never `>= distk`: see the one-block form above)
                    }
                    surv = valid && (lb < T);
                }
                if (valid && !surv) ++n_skip;
                const unsigned long long bal = __ballot(surv);
                const uint32_t mask32 = (uint32_t)(bal >> (half * 32));
                if (l32 == 0) s_mask[buf * kTB + bi] = mask32;
                if (surv) {
                    const uint32_t e = buf * kTC + bi * 32u + l32;
                    q_slot[e] = slot;
                    q_lb[e] = lb;
                    q_ip[e] = ip;
                    q_gadd[e] = m_c[i].g_add;
                    q_d[e] = est;
                }
            }
          }
            STAMP(st_a);
            lds_barrier(); // A: this tile is published to the replay wave
#ifdef RBQ_STAMPS
            STAMP(st_b); st_waitA += st_b - st_a;
#endif
            if (fast && s_restart) break; // a tie was met: leave the pass now (every wave reads the flag behind the same barrier)
            uint32_t S = 0;
#pragma unroll
            for (int j = 0; j < kTB; ++j) S += __popc(s_mask[buf * kTB + j]);
#ifdef RBQ_STAMPS
            st_surv += S;
#endif
            if (S > kLightMax) { // synchronous tile: help refining round by round, then use the fresh threshold
                STAMP(st_a);
                while (true) {
                    lds_barrier(); // B_r: this round's refine batch (or the end marker) is published
                    const uint32_t nb = s_nbatch;
                    if (nb == kBatchDone) break;
#ifdef RBQ_STAMPS
                    ++st_rounds;
#endif
                    if (kDual) refine_pair(buf, nb & 0xffffu, tid >> 4, nb >> 16);
                    else {
                        refine_batch(buf, nb & 0xffffu, tid >> 4);
                        if (kHeavyPer == 2) refine_batch(buf, nb & 0xffffu, (tid >> 4) + (nb >> 16));
                    }
                    lds_barrier(); // C_r: refined distances visible to the replay wave
                }
#ifdef RBQ_STAMPS
                STAMP(st_b); st_heavy += st_b - st_a; ++st_nheavy;
#endif
            }
        } else {
            // ---------------------------------------------------------------- replay wave (uniform control flow)
            STAMP(r0);
            if (tie_pending && !tlog && lane == 0) s_restart = 1u; // (with a tie log the pass runs to its end: the log must be complete)
            lds_barrier(); // A
            RSTAMP(rp_waitA);
            if (fast && s_restart) break;
            // compaction in stream order: block by block, lane order within the block
            for (uint32_t b = half; b < (uint32_t)kTB; b += 2) {
                uint32_t base = 0;
                for (uint32_t j = 0; j < b; ++j) base += __popc(s_mask[buf * kTB + j]);
                const uint32_t m = s_mask[buf * kTB + b];
                if ((m >> l32) & 1u) s_list[base + __popc(m & ((1u << l32) - 1u))] = b * 32u + l32;
            }
            uint32_t S = 0;
#pragma unroll
            for (int j = 0; j < kTB; ++j) S += __popc(s_mask[buf * kTB + j]);
            S = __builtin_amdgcn_readfirstlane(S);
            const bool heavy = S > kLightMax;
            // Exact sequential replay of the reference's prune/push/pop loop in stream order, with LAZY refine:
            // a round takes the next survivors whose lb is below the CURRENT true threshold (a superset of the
            // ones the reference evaluates, since the threshold only shrinks), refines them in parallel and then
            // replays the examined stretch against the running threshold.
            uint32_t n_ref_tile = 0; // candidates taken for refinement in this tile (traffic counter)
            struct Batch { uint32_t p, np, ncol, e, logb; unsigned long long mt; int v_lb; };
            auto cur_distk = [&]() -> float {
                if (fast) return rh.len < top_k ? INFINITY : __int_as_float(!kRank ? SortedRun<TR>::kth(rh.hd, rh.xd, rh.len, top_k) : bag_dk);
                return reg_heap ? (rh.len < top_k ? INFINITY : __int_as_float(rh.d_at(0)))
                                : (lh.len < top_k ? INFINITY : heap_d[0]);
            };
            // next batch from position p: stretches without a wanted survivor are skipped (and counted) on the way;
            // the (at most G) wanted ones of the first stretch that has any go to s_batch
            auto collect = [&](uint32_t p, uint32_t G, float distk0) -> Batch {
                Batch bt;
                while (true) {
                    const uint32_t i = p + lane;
                    uint32_t e = 0;
                    float lbv = INFINITY;
                    if (i < S) { e = buf * kTC + s_list[i]; lbv = q_lb[e]; }
                    const bool want = i < S && lbv < distk0;
                    const unsigned long long m = __ballot(want);
                    uint32_t np = p + 64u < S ? p + 64u : S;
                    if (m == 0ull && np < S) { n_skip += np - p; p = np; continue; }
                    const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
                    const bool take = want && rank < G;
                    const unsigned long long mt = __ballot(take);
                    if ((uint32_t)__popcll(m) > G) np = p + (63u - (uint32_t)__builtin_clzll(mt)) + 1u; // stop after the G-th taken
                    if (ex_bits && take) s_batch[rank] = s_list[i];
                    n_ref_tile += (uint32_t)__popcll(mt);
                    bt.p = p; bt.np = np; bt.ncol = (uint32_t)__popcll(mt); bt.e = e; bt.mt = mt; bt.v_lb = __float_as_int(lbv);
                    bt.logb = log_n;
                    if (tlog && fast) log_n += bt.ncol; // batches are collected in stream order (the replay may lag one batch behind)
                    return bt;
                }
            };
            // replay [bt.p, bt.np): only the taken survivors can pass the running threshold (it never grows, so
            // lb >= distk0 stays pruned); the rest of the stretch is counted as skipped in one step
            auto replay = [&](const Batch& bt) {
                int v_d = 0;
                uint32_t v_s = 0;
                if ((bt.mt >> lane) & 1ull) { v_d = __float_as_int(q_d[bt.e]); v_s = q_slot[bt.e]; }
                unsigned long long todo = bt.mt;
                n_skip += (bt.np - bt.p) - bt.ncol;
                if (tlog && fast) { // tie log: the batch's candidates, in stream order (one 12-byte store per taken lane)
                    const uint32_t at = bt.logb + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bt.mt >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bt.mt, 0u));
                    if (((bt.mt >> lane) & 1ull) && at < P.tie_log_cap) {
                        uint32_t* ent = tlog + at * 3u; // (three dword stores from one address: no register triple to find)
                        ent[0] = (uint32_t)bt.v_lb; ent[1] = (uint32_t)v_d; ent[2] = v_s;
                    }
                }
#if RBQ_STAMPS == 4
                asm volatile("s_waitcnt lgkmcnt(0)" :: "v"(v_d), "v"(v_s) : "memory");
                RSTAMP(rp_x1); // the batch's distances have arrived from LDS
#endif
                if (fast && kRank) {
                    // the whole batch in one data-parallel step (RankRun)
                    uint32_t c_skip = 0, c_ext = 0, c_est = 0;
                    int dk = bag_dk;
#ifdef RBQ_STAMPS
                    const bool serial_counts = false; // (the diag slots carry cycle stamps in this build)
#else
                    const bool serial_counts = count_skips;
#endif
                    const bool tie = RankRun<TR>::merge_batch(rh, top_k, bt.mt, bt.v_lb, v_d, v_s, lane, serial_counts,
                                                              reinterpret_cast<int*>(heap_d), heap_s, c_skip, c_ext, c_est, dk, kLazyTies, amb_min
#if RBQ_STAMPS == 4
                                                              , mst
#endif
                                                              );
                    bag_dk = dk;
                    n_skip += c_skip; n_ext += c_ext; n_est += c_est;
                    tie_pending |= tie; // published before the next barrier A (or F), so that every wave reads the same flag after it
#if RBQ_STAMPS == 4
                    RSTAMP(rp_x2); // the merge
#endif
                } else if (fast) {
                    // One taken survivor after the other, everything in scalar registers (all of it is wave-uniform:
                    // readlane / readfirstlane say so to the compiler): about a dozen instructions per survivor that does
                    // not change the top-k, the insertion on top for the ones that do.
                    uint32_t len_s = HeapOps::uni(rh.len);
                    bool tie = false;
                    int dk = SortedRun<TR>::kth(rh.hd, rh.xd, len_s, top_k);
                    uint32_t c_skip = 0, c_ext = 0, c_est = 0;
                    if (!count_skips && len_s == top_k) {
                        // One data-parallel test in front of the serial loop (lane j = candidate j): the threshold only falls
                        // inside the batch, so a candidate whose lower bound or whose distance is not below the threshold
                        // at the START of the batch is skipped or rejected by the reference as well (an EQUAL distance stays in:
                        // the serial loop must report the tie).  Once the run is full most of a batch ends here.
                        const int kk0 = HeapOps::key(dk);
                        const bool pass = (bt.mt >> lane) & 1ull && __int_as_float(bt.v_lb) < __int_as_float(dk) &&
                                          (v_d & 0x7f800000) != 0x7f800000 && HeapOps::key(v_d) <= kk0;
                        todo = __ballot(pass);
                    }
                    while (todo) {
                        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        const float lb = __int_as_float(__builtin_amdgcn_readlane(bt.v_lb, (int)j));
                        if (!(lb < __int_as_float(dk))) { ++c_skip; continue; }   // `lower_bound >= distk`: skipped
                        ++c_ext;
                        const int dbits = __builtin_amdgcn_readlane(v_d, (int)j);
                        if ((dbits & 0x7f800000) == 0x7f800000) continue;          // non-finite distance: dropped
                        ++c_est;
                        const int ke = HeapOps::key(dbits);
                        const bool was_full = len_s == top_k;
                        const int kk = HeapOps::key(dk);
                        if (was_full) {
                            if (ke > kk) continue;                                  // pushed and popped again: no change
                            if (ke == kk) { // turned away with the maximum's key: which of the equal maxima leaves depends on the heap layout
                                if (kLazyTies) amb_min = amb_min < kk ? amb_min : kk; else tie = true;
                                continue;
                            }
                        }
                        const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)v_s, (int)j);
                        const bool eqk = SortedRun<TR>::insert(rh.hd, rh.hs, rh.xd, rh.xs, len_s, dbits, slot, lane); // (lazy: equal keys side by side)
                        if (!kLazyTies) tie |= eqk;
                        len_s = len_s < top_k ? len_s + 1u : len_s; // a full run drops its (new) entry top_k
                        dk = SortedRun<TR>::kth(rh.hd, rh.xd, len_s, top_k);
                        if (kLazyTies && was_full && HeapOps::key(dk) == kk) amb_min = amb_min < kk ? amb_min : kk; // the old maximum left, its twin stays
                    }
                    rh.len = len_s;
                    n_skip += c_skip; n_ext += c_ext; n_est += c_est;
                    tie_pending |= tie; // published before the next barrier A (or F), so that every wave reads the same flag after it
                } else if (reg_heap) {
                    while (todo) {
                        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        const float lb = __int_as_float(__builtin_amdgcn_readlane(bt.v_lb, (int)j));
                        const float distk = rh.len < top_k ? INFINITY : __int_as_float(rh.d_at(0));
                        if (lb >= distk) { ++n_skip; continue; }
                        ++n_ext;
                        const int dbits = __builtin_amdgcn_readlane(v_d, (int)j);
                        if (!finite_f(__int_as_float(dbits))) continue;
                        ++n_est;
                        rh.push(dbits, (uint32_t)__builtin_amdgcn_readlane((int)v_s, (int)j));
                        if (rh.len > top_k) rh.pop();
                    }
                } else {
                    while (todo) { // uniform values, heap in LDS (top_k >= 64)
                        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        const float lb = __int_as_float(__builtin_amdgcn_readlane(bt.v_lb, (int)j));
                        const float distk = lh.len < top_k ? INFINITY : heap_d[0];
                        if (lb >= distk) { ++n_skip; continue; }
                        ++n_ext;
                        const float d = __int_as_float(__builtin_amdgcn_readlane(v_d, (int)j));
                        if (!finite_f(d)) continue;
                        ++n_est;
                        if (lane == 0) {
                            lh.push(d, (uint32_t)__builtin_amdgcn_readlane((int)v_s, (int)j));
                            if (lh.len > top_k) lh.pop();
                        }
                        lh.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)lh.len);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        if (P.heap_ws) __threadfence_block(); // (global heap: lane 0's stores before the wave reads the root again)
                    }
                }
            };
            if (!(heavy && ex_bits)) {
                // light tile (or no ex codes): the wave refines with its own 4 groups while the scanners go on
                const uint32_t G = ex_bits ? (kDual ? 8u : 4u) : 64u;
                uint32_t p = 0;
                while (p < S) {
                    const Batch bt = collect(p, G, cur_distk());
                    if (ex_bits && bt.ncol) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        if (kDual) refine_pair(buf, bt.ncol, lane >> 4, 4u);
                        else refine_batch(buf, bt.ncol, lane >> 4);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    }
                    replay(bt);
                    p = bt.np;
                }
                RSTAMP(rp_light);
            } else {
                // heavy tile, software-pipelined: round 0 is refined by all 16 groups; from then on the scanners'
                // 12 groups refine batch r+1 — collected with the threshold as it stands BEFORE batch r is
                // replayed, i.e. a superset again — while this wave replays batch r.
                STAMP(r0);
                constexpr uint32_t kPer = kDual ? 2u : (uint32_t)kHeavyPer; // survivors per 16-lane group and round
                Batch cur = collect(0, kPer * (uint32_t)(kScanThreads / 16), cur_distk());
                RSTAMP(rp_collect);
                if (lane == 0) s_nbatch = cur.ncol | ((uint32_t)(kScanThreads / 16) << 16); // batch size | groups
                lds_barrier(); // B_0
                if (kDual) refine_pair(buf, cur.ncol, tid >> 4, (uint32_t)(kScanThreads / 16));
                else {
                    refine_batch(buf, cur.ncol, tid >> 4);
                    if (kHeavyPer == 2) refine_batch(buf, cur.ncol, (tid >> 4) + (uint32_t)(kScanThreads / 16));
                }
                lds_barrier(); // C_0
                RSTAMP(rp_ref0);
                while (cur.np < S) {
                    const Batch nxt = collect(cur.np, kPer * (uint32_t)(kNScan * 4), cur_distk());
                    if (lane == 0) s_nbatch = nxt.ncol | ((uint32_t)(kNScan * 4) << 16);
                    lds_barrier(); // B_r: the scanners start on batch r+1
                    RSTAMP(rp_collect);
                    replay(cur);
                    RSTAMP(rp_replay);
                    lds_barrier(); // C_r
                    RSTAMP(rp_waitC);
                    cur = nxt;
                }
                replay(cur);
                RSTAMP(rp_replay);
            }
            {
                const float tnew = cur_distk();
                if (lane == 0) {
                    s_T = tnew;
                    if (ex_bits && P.prof) s_misc[7] += n_ref_tile;
                }
            }
            if (heavy) {
                if (lane == 0) s_nbatch = kBatchDone;
                lds_barrier(); // final B: helpers leave the tile, fresh T is visible
            }
        }
#ifdef RBQ_STAMPS
        STAMP(st_b); st_tiles += st_b - st_t0;
#endif
        qhead = (qhead + n) % kQueueCap;
        qcount -= n;
        ++tile;
    }
    if (kLazyTies && !scanner && fast && !tie_pending) { // the final look of the lazy-tie rule (k_scanw's, same registers)
        const uint32_t lenf = HeapOps::uni(rh.len);
        bool eq = false;
        int maxkey = (int)0x80000000;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const uint32_t i = (uint32_t)r * 64u + lane;
            const int b = r == 0 ? rh.hd : rh.xd[r];
            const int kv = kRank ? b : HeapOps::key(b);
            int below = __builtin_amdgcn_update_dpp((int)0x80000000, kv, 0x138, 0xf, 0xf, false); // wave_shr:1
            if (r > 0) {
                const int pb = r == 1 ? rh.hd : rh.xd[r - 1];
                const int carry = __builtin_amdgcn_readlane(kRank ? pb : HeapOps::key(pb), 63);
                below = lane == 0 ? carry : below;
            }
            eq |= i >= 1u && i < lenf && kv == below;
            if (lenf && (lenf - 1u) >> 6 == (uint32_t)r) maxkey = __builtin_amdgcn_readlane(kv, (int)((lenf - 1u) & 63u));
        }
        tie_pending = __ballot(eq) != 0ull || (lenf == top_k && maxkey == amb_min);
    }
    if (!scanner && fast && tie_pending && tlog && log_n <= P.tie_log_cap) {
        // the tied query: the reference's loop over the logged candidates with the BinaryHeap emulation (this wave alone; the
        // scanners wait at barrier F).  The heap ends up where the re-scan would have left it.  (Not inlined: the cold path must not
        // take part in the register allocation of the scan loop — it cost the top_k = 100 instantiation a spill inside every tile.)
        __threadfence_block(); // (the log was written by this wave: its stores are complete before the loads below)
        if (lane == 0 && P.heap_restarts) atomicAdd(P.heap_restarts, 1u);
        rh = tie_log_replay<TR>(heap_d, heap_s, tlog, log_n, top_k, reg_heap, lane, P.tie_stats);
        lh.len = rh.len;
        fast = false; // (this wave only: the result is read from the heap below)
        tie_pending = false;
    }
    if (tie_pending && lane == 0) { s_restart = 1u; if (tlog && P.tie_stats) atomicAdd(P.tie_stats + 3, 1u); } // (lazy ties: decided by the final run)
    lds_barrier(); // F: the replay wave has consumed the last tile
    if (!s_restart) break;
    __syncthreads(); // every wave has seen the flag
    if (tid == 0) {
        s_T = INFINITY; s_restart = 0;
        if (P.heap_restarts) atomicAdd(P.heap_restarts, 1u);
    }
    fast = false;
    pos = 0; qhead = 0; qcount = 0; tile = 0; win = (uint32_t)(RBQ_WIN0);
    ++p_pass;
    n_skip = 0; n_ext = 0; n_est = 0;
    rh.len = 0;
    bag_dk = 0x7f800000;
    tie_pending = false;
    amb_min = 0x7fffffff;
    __syncthreads();
  }
    if (!scanner) {
        if (fast) { // the sorted run: already ascending (TR > 1: keys)
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t i = (uint32_t)r * 64u + lane;
                if (i < rh.len) {
                    const int dv = r == 0 ? rh.hd : rh.xd[r];
                    heap_d[i] = __int_as_float(!kRank ? dv : HeapOps::key(dv));
                    heap_s[i] = r == 0 ? rh.hs : rh.xs[r];
                }
            }
            if (lane == 0) s_len = rh.len;
        } else {
        if (reg_heap) { // spill the register heap to LDS for the final heap-sort
#pragma unroll
            for (int r = 0; r < TR; ++r)
                if ((uint32_t)r * 64u + lane < rh.len) {
                    heap_d[r * 64 + lane] = __int_as_float(r == 0 ? rh.hd : rh.xd[r]);
                    heap_s[r * 64 + lane] = r == 0 ? rh.hs : rh.xs[r];
                }
            lh.len = rh.len;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (lane == 0) {
            lh.into_sorted();
            s_len = lh.len;
        }
        if (P.heap_ws) __threadfence_block(); // (global heap: visible to the other waves behind the barrier below)
        }
        if (lane != 0) { n_skip = 0; n_ext = 0; n_est = 0; } // uniform counters: report them once
    }

    if (P.diag && n_skip) atomicAdd(s_nskip, n_skip);
    if (P.prof && scanner && l32 == 0 && p_meta) { atomicAdd(&s_misc[5], p_code); atomicAdd(&s_misc[6], p_meta); }
    __syncthreads();
    if (P.prof) {
        if (tid == 0) {
            unsigned long long* pc = P.prof + prof_stripe(q);
            atomicAdd(pc + kProfCodeBlocks, (unsigned long long)s_misc[5]);
            atomicAdd(pc + kProfMetaBlocks, (unsigned long long)s_misc[6]);
            atomicAdd(pc + kProfStreamEntries, (unsigned long long)ns * p_pass);
            atomicAdd(pc + kProfQueries, 1ull);
        }
        if (wave == (uint32_t)kNScan && lane == 0 && ex_bits) atomicAdd(P.prof + prof_stripe(q) + kProfExEvals, (unsigned long long)s_misc[7]);
    }
    const uint32_t len = s_len;
    for (uint32_t i = tid; i < top_k; i += kScanThreads) {
        uint64_t id = ~0ull;
        float sc = __int_as_float(0x7fc00000);
        if (i < len) {
            id = P.ids[heap_s[i]];
            sc = (P.metric == 0 || P.mstg) ? heap_d[i] : -heap_d[i]; // MSTG reports the distance for both metrics
        }
        P.out_ids[(size_t)q * top_k + i] = id;
        P.out_scores[(size_t)q * top_k + i] = sc;
    }
#ifdef RBQ_STAMPS
#if RBQ_STAMPS == 3
    if (tid == 0 && P.diag) { // scanner wave 0: lookup time, wait at barrier A, live tiles
        P.diag[(size_t)q * 3 + 0] = (st_look & 0xffffffffull) | (st_waitA << 32);
        P.diag[(size_t)q * 3 + 1] = (unsigned long long)(st_ntile - st_dead) | ((unsigned long long)st_surv << 32);
        P.diag[(size_t)q * 3 + 2] = (st_fill & 0xffffffffull) | ((unsigned long long)st_nheavy << 32);
    }
#endif
    if (RBQ_STAMPS == 1 && tid == 0 && P.diag) { // diagnostic build: the diag slots carry cycle stamps of scanner wave 0 instead
        const unsigned long long st_total0 = st_total;
        st_total = __builtin_amdgcn_s_memtime() - st_total;
        P.diag[(size_t)q * 3 + 0] = (st_heavy & 0xffffffffull) | ((unsigned long long)st_rounds << 32);
        P.diag[(size_t)q * 3 + 1] = (st_total & 0xffffffffull) | (((st_loop0 - st_total0) & 0xffffull) << 32) | ((unsigned long long)(tile & 0xffff) << 48);
        P.diag[(size_t)q * 3 + 2] = (unsigned long long)(st_tiles & 0xffffffffull) | (st_fill << 32);
    }
    if (wave == (uint32_t)kNScan && lane == 0) {
        P.out_counts[q] = len;
#if RBQ_STAMPS == 4
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = (rp_x1 & 0xffffffffull) | (rp_x2 << 32);
            P.diag[(size_t)q * 3 + 1] = (mst[0] & 0xffffffffull) | (mst[1] << 32);
            P.diag[(size_t)q * 3 + 2] = (mst[2] & 0xffffffffull) | (rp_waitA << 32);
        }
#endif
#if RBQ_STAMPS == 2
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = (rp_collect & 0xffffffffull) | (rp_ref0 << 32);
            P.diag[(size_t)q * 3 + 1] = (rp_replay & 0xffffffffull) | (rp_waitC << 32);
            P.diag[(size_t)q * 3 + 2] = (rp_light & 0xffffffffull) | (rp_waitA << 32);
        }
#endif
    }
    if (false) {
#else
    if (wave == (uint32_t)kNScan && lane == 0) {
#endif
        P.out_counts[q] = len;
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = n_est;
            // + the vectors of probed lists that the probe selection proved skipped as a whole (never streamed)
            P.diag[(size_t)q * 3 + 1] = *s_nskip + (P.dead_skipped ? P.dead_skipped[q] : 0u);
            P.diag[(size_t)q * 3 + 2] = ex_bits ? n_ext : 0;
        }
    }
}

} // namespace rbq
