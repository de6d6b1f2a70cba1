// query_kernels.hpp — the kernels of the query stages in front of the scan that are not templates on the GEMM shape:
// k_prep / k_prep_wave (rotate + constants + LUT) and k_rank_scores (the all-pairs canonical ranking kept as the exact_rank option;
// its selection, k_select, is in select_given.hpp).  Included by k_query.hip only.
//
// Query preparation has three kernels: k_prep and k_prep_wave here, k_lat_front in latency.hpp.  What they compute is ONE copy of
// device functions — rotate_by_wave, store_rotated (the rotated query, its GEMM image, the f16 residual), lut_entries,
// lut_key_range, lut_quantise, lut_store, query_consts (with ex_dot_range and f16_resid_norm) — so their outputs agree bit for bit by
// construction.  What differs is structure, measured and kept per kernel: who rotates and which barriers exist, the form of the
// strictly sequential sums, how ranges and sums are reduced (LDS atomics or wave shuffles), and where the positive / negative sums
// are taken: serially on one thread in k_prep, strided per lane and a xor tree in the other two, so q1norm, exlo and exhi of k_prep
// differ from theirs in the last bits (tests/test_gpu_prep_kernels_agree.py holds all of this together on one input).
#pragma once
#include "kernels.hpp"

namespace rbq {

// Range of sum_i code_i * q_i over ALL ex codes (code_i in [0, 2^ex - 1]) from the sums of the positive and of the negative
// query elements, widened by 1e-3 of the largest possible magnitude: that covers the rounding of these two sums and of the
// scan kernel's own 16-lane FMA summation (each below D * 2^-24 <= 1.3e-4 relative for D <= 2048).  The other numeric
// variants' orders are covered by the same slack: the AVX2 order is 8 FMA chains of D / 8 steps and a 3-level tree (below
// D * 2^-24 as well); the portable order (kernels.hpp, ex_dot_var) rounds each of the D products once and then adds them in
// one serial chain, which is at most (D + 1) * 2^-24 of the sum of |terms| — 1.2e-4 at D = 2048, still below 1e-3.
__device__ __forceinline__ void ex_dot_range(float sum_pos, float sum_neg, uint32_t ex_bits, float& lo, float& hi) {
    const float cmax = (float)((1u << ex_bits) - 1u);
    const float slack = cmax * (sum_pos - sum_neg) * 1e-3f;
    lo = cmax * sum_neg - slack;
    hi = cmax * sum_pos + slack;
}

// |q - f16(q)| of a query image from n partial sums of its squared element residuals (f64: the squares are exact, the sum is good to
// 2^-53 per term), the root rounded up; not finite when the image is not
__device__ __forceinline__ float f16_resid_norm(const double* part, int n) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) a += part[i];
    return (float)(sqrt(a) * 1.000001);
}

// In-register FHT of one wave over n = 64*EPL floats at `part` (LDS): lane holds elements lane*EPL .. +EPL-1, so
// the stages h < EPL are register butterflies and the stages h = EPL*m (m = 1..32) exchange with lane ^ m.  Same
// butterflies in the same stage order as fht_lds (out[j] = x[j] + x[j+h], out[j+h] = x[j] - x[j+h]), followed by
// the reference's rescale x * fac.
// value of lane ^ M: DPP inside a row of 16 lanes (quad_perm for 1 and 2; row_shl:4 / row_shr:4 on alternate quads for 4;
// row_ror:8 for 8), gfx950's v_permlane16_swap / v_permlane32_swap between rows and halves (semantics probed with
// tests/diag/micro/permlane_probe.hip) — no LDS round trip (the first form used ds_bpermute for every stage: 48 of them
// per transform, with one wave per SIMD every one of their latencies was exposed)
template <int M>
__device__ __forceinline__ float lane_xor(float v, uint32_t lane) {
    const int vi = __float_as_int(v);
    if (M == 1) return __int_as_float(__builtin_amdgcn_update_dpp(vi, vi, 0xB1, 0xf, 0xf, false)); // quad_perm [1,0,3,2]
    if (M == 2) return __int_as_float(__builtin_amdgcn_update_dpp(vi, vi, 0x4E, 0xf, 0xf, false)); // quad_perm [2,3,0,1]
    if (M == 4) {
        int t = __builtin_amdgcn_update_dpp(vi, vi, 0x104, 0xf, 0x5, false);                       // quads 0,2 <- lane + 4
        t = __builtin_amdgcn_update_dpp(t, vi, 0x114, 0xf, 0xa, false);                            // quads 1,3 <- lane - 4
        return __int_as_float(t);
    }
    if (M == 8) return __int_as_float(__builtin_amdgcn_update_dpp(vi, vi, 0x128, 0xf, 0xf, false)); // row_ror:8
    if (M == 16) { // r[0] = rows {0,0,2,2} of v, r[1] = rows {1,1,3,3}
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)vi, (unsigned)vi, false, false);
        return __int_as_float((int)((lane & 16u) ? r[0] : r[1]));
    }
    // M == 32: r[0] = the lower half twice, r[1] = the upper half twice
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)vi, (unsigned)vi, false, false);
    return __int_as_float((int)((lane & 32u) ? r[0] : r[1]));
}

// stage h = EPL * M of the transform for this lane's EPL elements: lower partner x + y, upper partner x - y (= p + (-v))
template <int EPL, int M>
__device__ __forceinline__ void fht_exchange(float (&v)[EPL], uint32_t lane) {
    const bool upper = (lane & (uint32_t)M) != 0;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
        const float p = lane_xor<M>(v[k], lane);
        const float sv = upper ? -v[k] : v[k];
        v[k] = p + sv;
    }
}

// `flip` != null: the flip-sign bits of the elements of `part` (LSB-first, bit i = element i), applied as the elements are
// loaded (flip_sign of the round fused into the transform's own read: no separate pass over the vector)
template <int EPL>
__device__ __forceinline__ void fht_wave(float* part, uint32_t lane, float fac, const uint8_t* flip = nullptr) {
    float v[EPL];
    if (EPL >= 4) {
#pragma unroll
        for (int k = 0; k < EPL; k += 4) {
            const float4 t = *reinterpret_cast<const float4*>(part + lane * EPL + k);
            v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) v[k] = part[lane * EPL + k];
    }
    if (flip) {
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            const uint32_t i = lane * EPL + k;
            if ((flip[i >> 3] >> (i & 7u)) & 1u) v[k] = -v[k];
        }
    }
#pragma unroll
    for (int h = 1; h < EPL; h <<= 1)
#pragma unroll
        for (int k = 0; k < EPL; ++k)
            if ((k & h) == 0) {
                const float a = v[k], b = v[k + h];
                v[k] = a + b;
                v[k + h] = a - b;
            }
    fht_exchange<EPL, 1>(v, lane);
    fht_exchange<EPL, 2>(v, lane);
    fht_exchange<EPL, 4>(v, lane);
    fht_exchange<EPL, 8>(v, lane);
    fht_exchange<EPL, 16>(v, lane);
    fht_exchange<EPL, 32>(v, lane);
    if (EPL >= 4) {
#pragma unroll
        for (int k = 0; k < EPL; k += 4)
            *reinterpret_cast<float4*>(part + lane * EPL + k) = make_float4(v[k] * fac, v[k + 1] * fac, v[k + 2] * fac, v[k + 3] * fac);
    } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) part[lane * EPL + k] = v[k] * fac;
    }
}

// FhtKacRotator::rotate_into by one wave; `flips` = the 4*D/8 flip-sign bytes (LDS copy).  Same operations on the same
// values as rotate_into_lds<64> (src/rotation.rs:350-401), with fht_wave in place of the LDS butterflies and the sign flips
// and the final scale FUSED into the passes next to them (a negation commutes with nothing else here: it is applied to
// the very value the separate pass would have negated): round 0's flips by the initial load, round r+1's flips by the
// Kac step of round r as it writes (or, for power-of-two dimensions, by the transform as it reads), the closing * 0.25
// by the last Kac step.  Per round the vector makes 4 passes through LDS as 16-byte accesses instead of 6 as scalars:
// the rotation was 17 of the 27 us of a single query's preparation.
// The initial load (with round 0's flips unless the dimension is a power of two) — a separate step so that the caller can issue
// it BEFORE the barrier behind the copy of the flip bits into LDS: `flips0` may be the global table.
// QT: the element of the query row (float, RawF16, RawBf16: kernels.hpp).  16-bit rows: a row that starts
// 4-byte aligned is loaded two adjacent elements per 32-bit load (fhtkac_initial_load_pairs); a row that starts 2-byte aligned only
// (odd dim, a base offset by one element) keeps the loop below with one 16-bit load per element.  Same values into the same x[i].
template <typename QT>
__device__ __forceinline__ void fhtkac_initial_load_pairs(float* x, const QT* __restrict__ qin, uint32_t dim, uint32_t D, uint32_t trunc,
                                                          const uint8_t* __restrict__ flips0, uint32_t lane) {
    // lane l owns the element pairs (2l, 2l + 1) + 128 u: eight 32-bit loads are requested before the first LDS write, as below, and
    // cover 1024 elements; the writes are 8 bytes per lane at a stride of 8 bytes — conflict-free.  D is even, so a pair never
    // straddles D; it can straddle dim (odd dim): that last element is loaded alone, nothing behind the row is read.
    constexpr int KU = 8;
    for (uint32_t i0 = 2u * lane; i0 < D; i0 += 128 * KU) {
        uint32_t w[KU], f[KU];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const uint32_t i = i0 + 128u * u;
            w[u] = i + 1 < dim ? *reinterpret_cast<const uint32_t*>(qin + i) : (i < dim ? (uint32_t)qin[i].bits : 0u);
            f[u] = (trunc != D && i < D) ? (uint32_t)flips0[i >> 3] : 0u;
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const uint32_t i = i0 + 128u * u;
            if (i < D) {
                const float a = raw_widen(QT{(uint16_t)(w[u] & 0xffffu)}), b = raw_widen(QT{(uint16_t)(w[u] >> 16)});
                const uint32_t fb = f[u] >> (i & 7u); // (i is even: both bits lie in the one byte)
                *reinterpret_cast<float2*>(x + i) = make_float2((fb & 1u) ? -a : a, (fb & 2u) ? -b : b);
            }
        }
    }
}
template <typename QT>
__device__ __forceinline__ void fhtkac_initial_load(float* x, const QT* __restrict__ qin, uint32_t dim, uint32_t D, uint32_t trunc,
                                                    const uint8_t* __restrict__ flips0, uint32_t lane) {
    if constexpr (sizeof(QT) == 2) { // (uniform over the wave: one query per wave)
        if ((reinterpret_cast<uintptr_t>(qin) & 3u) == 0) return fhtkac_initial_load_pairs(x, qin, dim, D, trunc, flips0, lane);
    }
    // eight elements per lane are REQUESTED before the first is written to LDS: as a plain loop hipcc waited for every load in front
    // of its ds_write — D / 64 dependent global round trips (15 at D = 960) at the head of every query's preparation (round 5)
    constexpr int KU = 8;
    for (uint32_t i0 = lane; i0 < D; i0 += 64 * KU) {
        QT v[KU];
        uint32_t f[KU];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const uint32_t i = i0 + 64u * u;
            // (dim <= D)  16-bit rows: the load itself is unguarded — a lane beyond dim reads element 0 of its row and drops it below.
            // Behind a guard the compiler sinks the widening into the guarded block and waits there for every single load: eight
            // dependent round trips per round, what this function exists to avoid (seen in the ISA)
            if constexpr (sizeof(QT) == 2) v[u] = qin[i < dim ? i : 0u];
            else v[u] = i < dim ? qin[i] : QT{};
            f[u] = (trunc != D && i < D) ? (uint32_t)flips0[i >> 3] : 0u;
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const uint32_t i = i0 + 64u * u;
            float w = raw_widen(v[u]);
            if constexpr (sizeof(QT) == 2) w = i < dim ? w : 0.0f;
            if (i < D) x[i] = ((f[u] >> (i & 7u)) & 1u) ? -w : w;
        }
    }
}
template <int EPL>
__device__ __forceinline__ void rotate_fhtkac_wave(float* x, uint32_t D, const uint8_t* flips, float fac, uint32_t lane) {
    constexpr uint32_t trunc = 64u * EPL;
    const uint32_t fo = D / 8, start = D - trunc, half = D / 2;
    group_sync<64>(); // (fhtkac_initial_load)
    if (trunc == D) { // 4 x (flip, transform of everything, scale)
        for (int r = 0; r < 4; ++r) {
            fht_wave<EPL>(x, lane, fac, flips + r * fo);
            group_sync<64>();
        }
        return;
    }
    for (int r = 0; r < 4; ++r) {
        fht_wave<EPL>((r & 1) ? x + start : x, lane, fac);
        group_sync<64>();
        // Kac step, four pairs (i, i + half) per lane and step; then the next round's flips, or the closing scale
        const uint8_t* fn = flips + (r + 1) * fo;
        for (uint32_t i = 4 * lane; i < half; i += 256) { // half % 32 == 0
            const float4 a = *reinterpret_cast<const float4*>(x + i), b = *reinterpret_cast<const float4*>(x + i + half);
            float s[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}, d[4] = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
            if (r < 3) {
                const uint32_t fs = (uint32_t)fn[i >> 3] >> (i & 7u), fd = (uint32_t)fn[(i + half) >> 3] >> ((i + half) & 7u); // (i, half: multiples of 4)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if ((fs >> k) & 1u) s[k] = -s[k];
                    if ((fd >> k) & 1u) d[k] = -d[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) { s[k] = s[k] * 0.25f; d[k] = d[k] * 0.25f; }
            }
            *reinterpret_cast<float4*>(x + i) = make_float4(s[0], s[1], s[2], s[3]);
            *reinterpret_cast<float4*>(x + i + half) = make_float4(d[0], d[1], d[2], d[3]);
        }
        group_sync<64>();
    }
}

// pack_lut_f32 entries of one codebook: lut[j] = lut[j - lowbit(j)] + q[KPOS[j]],  KPOS = {3,3,2,3,1,3,2,3,0,3,2,3,1,3,2,3}
__device__ __forceinline__ void lut_entries(const float* x4, float (&l)[16]) {
    const float q0 = x4[0], q1 = x4[1], q2 = x4[2], q3 = x4[3];
    l[0] = 0.0f;
    l[1] = l[0] + q3;
    l[2] = l[0] + q2;
    l[3] = l[2] + q3;
    l[4] = l[0] + q1;
    l[5] = l[4] + q3;
    l[6] = l[4] + q2;
    l[7] = l[6] + q3;
    l[8] = l[0] + q0;
    l[9] = l[8] + q3;
    l[10] = l[8] + q2;
    l[11] = l[10] + q3;
    l[12] = l[8] + q1;
    l[13] = l[12] + q3;
    l[14] = l[12] + q2;
    l[15] = l[14] + q3;
}

// ---- the steps the three preparation kernels share (k_prep and k_prep_wave below, k_lat_front in latency.hpp) ----

// DynamicRotator::rotate (src/rotation.rs:350-401) of the query at x (LDS) by ONE wave, for the FHT-Kac (`flips`: the LDS copy of its
// flip bits; the caller has run fhtkac_initial_load) and the identity rotator
template <typename QT>
__device__ __forceinline__ void rotate_by_wave(float* x, const QT* qin, uint32_t dim, uint32_t D, int rotator, const uint8_t* rot_blob,
                                               const uint8_t* flips, uint32_t trunc, float fac, uint32_t lane) {
    if (rotator == 1) {
        switch (trunc) {
            case 64: rotate_fhtkac_wave<1>(x, D, flips, fac, lane); break;
            case 128: rotate_fhtkac_wave<2>(x, D, flips, fac, lane); break;
            case 256: rotate_fhtkac_wave<4>(x, D, flips, fac, lane); break;
            case 512: rotate_fhtkac_wave<8>(x, D, flips, fac, lane); break;
            case 1024: rotate_fhtkac_wave<16>(x, D, flips, fac, lane); break;
            case 2048: rotate_fhtkac_wave<32>(x, D, flips, fac, lane); break;
            // dim < 64 (transform shorter than a wavefront) or >= 4096: the generic LDS butterflies
            default: rotate_into_lds<64>(x, nullptr, qin, dim, D, rotator, flips, trunc, fac, lane); break;
        }
    } else {
        rotate_into_lds<64>(x, nullptr, qin, dim, D, rotator, rot_blob, trunc, fac, lane);
    }
}

// element i of query q's rotated vector, and of its image for the ranking GEMM; rr collects the squared residual of the f16 image
__device__ __forceinline__ void store_rotated(float v, uint32_t q, uint32_t i, uint32_t D, float* rot_out, uint16_t* rot_hl, bool f16, double& rr) {
    rot_out[(size_t)q * D + i] = v;
    if (f16) { // one-product f16 image [nq][D] for k_rank_f16_db and its residual
        float r;
        rot_hl[(size_t)q * D + i] = f16_image(v, r);
        rr += (double)r * (double)r;
    } else if (rot_hl) { // split-bf16 image for k_rank_bf16_db (hi | lo per K slab: hl_offset)
        uint16_t h, l;
        bf16_split(v, h, l);
        rot_hl[(size_t)q * 2 * D + hl_offset(i, 0, D)] = h;
        rot_hl[(size_t)q * 2 * D + hl_offset(i, 1, D)] = l;
    }
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// QueryLut::new, pass 1: the value range of a codebook's entries, as total-order keys
__device__ __forceinline__ void lut_key_range(const float (&l)[16], int& kmin, int& kmax) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = total_key(l[j]);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
}
// pass 2: the sixteen u8 entries of a codebook (four dwords) and the smallest / largest of them
__device__ __forceinline__ uint4 lut_quantise(const float (&l)[16], float vl, float delta, uint32_t& emin, uint32_t& emax) {
    uint32_t w[4] = {0, 0, 0, 0};
    emin = 255; emax = 0;
    if (delta > 0.0f) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float v = roundf((l[j] - vl) / delta);
            v = v >= 0.0f ? v : 0.0f; // also maps NaN -> 0 like `as u8`
            v = v > 255.0f ? 255.0f : v;
            const uint32_t e = (uint32_t)v;
            emin = e < emin ? e : emin;
            emax = e > emax ? e : emax;
            w[j >> 2] |= e << (8 * (j & 3));
        }
    } else {
        emin = 0;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// device LUT order: adjacent codebooks swapped (position p holds codebook p^1) so that nibble m of a little-endian code dword
// indexes table (8*dword + m) directly; the code-layout padding (D not a multiple of 64) holds all-zero tables
__device__ __forceinline__ void lut_store(uint8_t* lut_out, uint32_t q, uint32_t Dc, uint32_t c, uint4 w) {
    *reinterpret_cast<uint4*>(lut_out + (size_t)q * Dc * 4 + (size_t)(c ^ 1u) * 16) = w;
}

// -DRBQ_PREP_STAMPS: the clock at the three phase boundaries of a preparation kernel; query_consts reports the phases' cycles in
// place of exlo / exhi / q1norm (lazy selection is off in this build)
struct PrepStamps {
#ifdef RBQ_PREP_STAMPS
    unsigned long long t[3];
    __device__ __forceinline__ void mark(int i) { t[i] = __builtin_amdgcn_s_memtime(); }
#else
    __device__ __forceinline__ void mark(int) {}
#endif
};

// QueryPrecomputed::new (src/ivf.rs:862-878) and the constants of QueryLut::new from the query's sums: s_sum and s_n2 the strictly
// sequential ones, sp / sn the sums of the positive / negative elements (ex_dot_range), amin / amax over the codebooks
__device__ __forceinline__ QueryConsts query_consts(uint32_t amin, uint32_t amax, float delta, float vl, uint32_t D, float s_sum, float s_n2,
                                                    float sp, float sn, uint32_t ex_bits, const PrepStamps& ps) {
    QueryConsts qc;
    qc.amin = (float)amin;
    qc.amax = (float)amax;
    qc.delta = delta;
    qc.sum_vl = vl * (float)(D / 4);
    qc.qnorm = sqrtf(s_n2);
    qc.qnorm2 = s_n2; qc.q1norm = (sp - sn) * 1.001f;
    ex_dot_range(sp, sn, ex_bits, qc.exlo, qc.exhi);
#ifdef RBQ_PREP_STAMPS
    qc.exlo = (float)(ps.t[1] - ps.t[0]); qc.exhi = (float)(ps.t[2] - ps.t[1]); qc.q1norm = (float)(__builtin_amdgcn_s_memtime() - ps.t[2]);
#endif
    qc.k1x = -0.5f * s_sum;
    const float cb = -((float)(1u << ex_bits) - 0.5f);
    qc.kbx = cb * s_sum;
    qc.scale = (float)(1u << ex_bits);
    return qc;
}

// One WORKGROUP per query, every rotator (the only kernel that serves the matrix rotator: O(D^2) per query).  Structure of its own:
// the whole workgroup rotates; the sequential sums run on three separate threads, the positive / negative sums among them, serially
// (so q1norm, exlo and exhi differ from the other two kernels' in the last bits); each thread keeps the entries of its (at most two)
// codebooks in registers across the barrier behind the range; ranges and u8 sums meet through LDS atomics.
// dynamic LDS: 2 x D floats (vector | matrix rotator input)
// QT (here and in k_prep_wave, k_lat_front): the element of the query rows, widened where the rotation loads it; nothing behind the
// rotation's input sees it
template <typename QT>
__global__ __launch_bounds__(kThreads) void k_prep(const QT* __restrict__ queries, uint32_t dim, uint32_t D,
                                                   uint32_t Dc, int rotator, const uint8_t* __restrict__ rot_blob,
                                                   uint32_t trunc, float fac, uint32_t ex_bits,
                                                   float* __restrict__ rot_out, uint8_t* __restrict__ lut_out,
                                                   QueryConsts* __restrict__ consts,
                                                   uint16_t* __restrict__ rot_hl, float* __restrict__ rank_resid) {
    extern __shared__ __align__(16) float sm[];
    __shared__ double s_rr[kThreads / 64]; // (one-product f16 route) squared residual of the image, per wave
    float* x = sm;         // [D]
    float* y = sm + D;     // [D] (matrix rotator input)
    __shared__ int s_kmin, s_kmax;
    __shared__ unsigned int s_amin, s_amax;
    __shared__ float s_sum, s_n2, s_pos, s_neg;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const QT* qin = queries + (size_t)q * dim;
    PrepStamps ps;
    ps.mark(0);

    rotate_into_lds<kThreads>(x, y, qin, dim, D, rotator, rot_blob, trunc, fac, tid);

    double rr = 0.0;
    for (uint32_t i = tid; i < D; i += kThreads) store_rotated(x[i], q, i, D, rot_out, rot_hl, rank_resid != nullptr, rr);
    if (rank_resid) { // (uniform) per-wave sums now, their total behind the barrier below
        rr = wave_sum(rr);
        if ((tid & 63u) == 0) s_rr[tid >> 6] = rr;
    }

    ps.mark(1);
    // QueryPrecomputed::new — strictly sequential sums (Rust iter().sum() folds from -0.0)
    if (tid == 0) {
        float s = -0.0f;
        for (uint32_t i = 0; i < D; ++i) s = s + x[i];
        s_sum = s;
        s_kmin = 0x7fffffff;
        s_kmax = (int)0x80000000;
        s_amin = 0;
        s_amax = 0;
    }
    if (tid == 64) {
        float n2 = -0.0f;
        for (uint32_t i = 0; i < D; ++i) {
            float p = x[i] * x[i];
            n2 = n2 + p;
        }
        s_n2 = n2;
    }
    if (tid == 128) { // sums of the positive / negative elements: range of the ex-code dot product (ex_dot_range)
        float sp = 0.0f, sn = 0.0f;
        for (uint32_t i = 0; i < D; ++i) { sp += fmaxf(x[i], 0.0f); sn += fminf(x[i], 0.0f); }
        s_pos = sp; s_neg = sn;
    }
    __syncthreads();
    if (rank_resid && tid == 0) rank_resid[q] = f16_resid_norm(s_rr, kThreads / 64);

    ps.mark(2);
    // pack_lut_f32 + QueryLut::new.  D <= 2048 -> at most 2 codebooks per thread.
    const uint32_t ncb = D / 4;
    float l[2][16];
    int kmin = 0x7fffffff, kmax = (int)0x80000000;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        uint32_t c = tid + u * kThreads;
        if (c < ncb) {
            lut_entries(x + 4 * c, l[u]);
            lut_key_range(l[u], kmin, kmax);
        }
    }
    atomicMin(&s_kmin, kmin);
    atomicMax(&s_kmax, kmax);
    __syncthreads();
    const float vl = key_to_float(s_kmin), vr = key_to_float(s_kmax);
    const float delta = (vr - vl) / 255.0f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        uint32_t c = tid + u * kThreads;
        if (c < ncb) {
            uint32_t emin, emax;
            const uint4 w = lut_quantise(l[u], vl, delta, emin, emax);
            atomicAdd(&s_amin, emin);
            atomicAdd(&s_amax, emax);
            lut_store(lut_out, q, Dc, c, w);
        } else if (c < Dc / 4) {
            lut_store(lut_out, q, Dc, c, make_uint4(0, 0, 0, 0));
        }
    }
    __syncthreads();
    if (tid == 0) consts[q] = query_consts(s_amin, s_amax, delta, vl, D, s_sum, s_n2, s_pos, s_neg, ex_bits, ps);
}

// One WAVE per query (4 queries per workgroup), FHT-Kac and identity rotators: the batch path.  Structure of its own: no workgroup
// barrier after the flip bits are in LDS — the butterflies synchronise through the wave's in-order LDS traffic; the positive /
// negative sums are taken strided per lane in the pass that writes the query and reduced by a xor tree, as are the range and the u8
// sums; the two strictly sequential sums (sum q, |q|^2: Rust iter().sum()) run side by side on lanes 0 and 1, 16 elements per step.
// dynamic LDS: 4 x 2 x D floats (vector + squares per wave) | 4*D/8 flip bytes
template <typename QT>
__global__ __launch_bounds__(kThreads) void k_prep_wave(const QT* __restrict__ queries, uint32_t nq, uint32_t dim, uint32_t D,
                                                        uint32_t Dc, int rotator, const uint8_t* __restrict__ rot_blob,
                                                        uint32_t trunc, float fac, uint32_t ex_bits,
                                                        float* __restrict__ rot_out, uint8_t* __restrict__ lut_out,
                                                        QueryConsts* __restrict__ consts,
                                                        uint16_t* __restrict__ rot_hl, float* __restrict__ rank_resid) {
    extern __shared__ __align__(16) float sm[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (kThreads / 64) + wave;
    uint8_t* flips = reinterpret_cast<uint8_t*>(sm + (size_t)2 * (kThreads / 64) * D); // 4*D/8 bytes (FHT-Kac)
    PrepStamps ps;
    ps.mark(0);
    float* x = sm + (size_t)wave * 2 * D;
    float* x2 = x + D; // squares, for the |q|^2 chain
    const QT* qin = queries + (size_t)q * dim;
    const bool wave_fht = rotator == 1 && trunc >= 64 && trunc <= 2048; // (else the generic LDS butterflies)
    if (rotator == 1) {
        for (uint32_t i = threadIdx.x; i < D / 8; i += kThreads) reinterpret_cast<uint32_t*>(flips)[i] = reinterpret_cast<const uint32_t*>(rot_blob)[i]; // (4 D / 8 flip bytes as dwords: one trip)
        // the query is requested together with the flip table (round 0's flips straight from the global table): one
        // round trip in front of the barrier instead of two around it
        if (q < nq && wave_fht) fhtkac_initial_load(x, qin, dim, D, trunc, rot_blob, lane);
        __syncthreads(); // the only workgroup barrier: before any wave can leave
    }
    if (q >= nq) return; // whole wave
    rotate_by_wave(x, qin, dim, D, rotator, rot_blob, flips, trunc, fac, lane);

    float sp = 0.0f, sn = 0.0f; // sums of the positive / negative elements (ex_dot_range)
    double rr = 0.0;            // (one-product f16 route) squared residual of the image
    for (uint32_t i = lane; i < D; i += 64) {
        const float v = x[i];
        x2[i] = v * v;
        sp += fmaxf(v, 0.0f);
        sn += fminf(v, 0.0f);
        store_rotated(v, q, i, D, rot_out, rot_hl, rank_resid != nullptr, rr);
    }
    if (rank_resid) { // (uniform)
        rr = wave_sum(rr);
        if (lane == 0) rank_resid[q] = f16_resid_norm(&rr, 1);
    }
    group_sync<64>();
    ps.mark(1);
    // QueryPrecomputed::new — strictly sequential sums (Rust iter().sum() folds from -0.0): lane 0 adds the
    // elements, lane 1 their squares
    float acc = -0.0f;
    if (lane < 2) { // 16 elements per step: four 16-byte LDS reads in flight, then the adds in element order
        const float* src = lane ? x2 : x;
        for (uint32_t i = 0; i < D; i += 16) { // D % 16 == 0
            float4 v4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v4[u] = *reinterpret_cast<const float4*>(src + i + 4 * u);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc = acc + v4[u].x;
                acc = acc + v4[u].y;
                acc = acc + v4[u].z;
                acc = acc + v4[u].w;
            }
        }
    }
    const float s_sum = __shfl(acc, 0, 64), s_n2 = __shfl(acc, 1, 64);

    ps.mark(2);
    // pack_lut_f32 + QueryLut::new: pass 1 finds the value range, pass 2 quantises
    const uint32_t ncb = D / 4;
    int kmin = 0x7fffffff, kmax = (int)0x80000000;
    for (uint32_t c = lane; c < ncb; c += 64) {
        float l[16];
        lut_entries(x + 4 * c, l);
        lut_key_range(l, kmin, kmax);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int a = __shfl_xor(kmin, d, 64), b = __shfl_xor(kmax, d, 64);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    const float vl = key_to_float(kmin), vr = key_to_float(kmax);
    const float delta = (vr - vl) / 255.0f;
    uint32_t amin = 0, amax = 0;
    for (uint32_t c = lane; c < Dc / 4; c += 64) {
        uint4 w = make_uint4(0, 0, 0, 0); // (padding codebook)
        if (c < ncb) {
            float l[16];
            lut_entries(x + 4 * c, l);
            uint32_t emin, emax;
            w = lut_quantise(l, vl, delta, emin, emax);
            amin += emin;
            amax += emax;
        }
        lut_store(lut_out, q, Dc, c, w);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        amin += __shfl_xor(amin, d, 64);
        amax += __shfl_xor(amax, d, 64);
        sp += __shfl_xor(sp, d, 64);
        sn += __shfl_xor(sn, d, 64);
    }
    if (lane == 0) consts[q] = query_consts(amin, amax, delta, vl, D, s_sum, s_n2, sp, sn, ex_bits, ps);
}

// ---------------------------------------------------------------------------------------------
// k_rank_scores: scores[q][c] = l2_distance_sqr(rot[q], cent[c]) or dot(...), in the reference's
// AVX2 lane order: 8 strided accumulators, unfused mul/add, lanes summed 0..7, scalar tail.
// Tile 32 queries x 32 centroids per workgroup, 2x2 pairs per thread, 32-dim LDS chunks.
// ---------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(kThreads) void k_rank_scores(const float* __restrict__ rot, const float* __restrict__ cent,
                                                          uint32_t nq, uint32_t nlist, uint32_t D,
                                                          float* __restrict__ scores) {
    __shared__ __align__(16) float Qs[32][36];
    __shared__ __align__(16) float Cs[32][36];
    const uint32_t tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
    const uint32_t q0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const uint32_t Dmain = D & ~7u;
    float acc[2][2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int l = 0; l < 8; ++l) acc[a][b][l] = 0.0f;

    const uint32_t lrow = tid >> 3, lcol = (tid & 7) * 4;
    for (uint32_t k0 = 0; k0 < Dmain; k0 += 32) {
        float4 qv = make_float4(0, 0, 0, 0), cv = make_float4(0, 0, 0, 0);
        const uint32_t k = k0 + lcol;
        if (q0 + lrow < nq) {
            const float* p = rot + (size_t)(q0 + lrow) * D + k;
            if (k + 4 <= Dmain && (D & 3) == 0) qv = *reinterpret_cast<const float4*>(p);
            else {
                if (k < Dmain) qv.x = p[0];
                if (k + 1 < Dmain) qv.y = p[1];
                if (k + 2 < Dmain) qv.z = p[2];
                if (k + 3 < Dmain) qv.w = p[3];
            }
        }
        if (c0 + lrow < nlist) {
            const float* p = cent + (size_t)(c0 + lrow) * D + k;
            if (k + 4 <= Dmain && (D & 3) == 0) cv = *reinterpret_cast<const float4*>(p);
            else {
                if (k < Dmain) cv.x = p[0];
                if (k + 1 < Dmain) cv.y = p[1];
                if (k + 2 < Dmain) cv.z = p[2];
                if (k + 3 < Dmain) cv.w = p[3];
            }
        }
        *reinterpret_cast<float4*>(&Qs[lrow][lcol]) = qv;
        *reinterpret_cast<float4*>(&Cs[lrow][lcol]) = cv;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float qa[2][8], cb[2][8];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float4 v0 = *reinterpret_cast<const float4*>(&Qs[2 * tq + a][8 * t]);
                float4 v1 = *reinterpret_cast<const float4*>(&Qs[2 * tq + a][8 * t + 4]);
                qa[a][0] = v0.x; qa[a][1] = v0.y; qa[a][2] = v0.z; qa[a][3] = v0.w;
                qa[a][4] = v1.x; qa[a][5] = v1.y; qa[a][6] = v1.z; qa[a][7] = v1.w;
                float4 w0 = *reinterpret_cast<const float4*>(&Cs[2 * tc + a][8 * t]);
                float4 w1 = *reinterpret_cast<const float4*>(&Cs[2 * tc + a][8 * t + 4]);
                cb[a][0] = w0.x; cb[a][1] = w0.y; cb[a][2] = w0.z; cb[a][3] = w0.w;
                cb[a][4] = w1.x; cb[a][5] = w1.y; cb[a][6] = w1.z; cb[a][7] = w1.w;
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int l = 0; l < 8; ++l) {
                        float p;
                        if (METRIC == 0) {
                            float d = qa[a][l] - cb[b][l];
                            p = d * d;
                        } else {
                            p = qa[a][l] * cb[b][l];
                        }
                        acc[a][b][l] = acc[a][b][l] + p;
                    }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const uint32_t qi = q0 + 2 * tq + a, ci = c0 + 2 * tc + b;
            if (qi < nq && ci < nlist) {
                float sum = 0.0f;
                if (Dmain > 0) {
                    sum = -0.0f;
#pragma unroll
                    for (int l = 0; l < 8; ++l) sum = sum + acc[a][b][l];
                }
                for (uint32_t i = Dmain; i < D; ++i) { // scalar tail
                    float x = rot[(size_t)qi * D + i], y = cent[(size_t)ci * D + i], p;
                    if (METRIC == 0) {
                        float d = x - y;
                        p = d * d;
                    } else {
                        p = x * y;
                    }
                    sum = sum + p;
                }
                scores[(size_t)qi * nlist + ci] = sum;
            }
        }
}

} // namespace rbq
