// encode_vec.hpp — k_encode: quantize_with_centroid (src/quantizer.rs:140-262, :264-308, :429-535) on the GPU, one THREAD
// per vector — every reduction of the reference is a sequential chain (iter().sum()) or the 8-accumulator AVX2 dot
// (src/math.rs:154-245), so a lane walks its vector in order while 64-dim tiles of 64 vectors are staged through LDS with
// coalesced loads.  Two passes over the rotated rows: the residual norm has to be known before the ex codes can be formed.
// A header of its own because two translation units instantiate the template: k_build.hip (the IVF device layout) and
// k_bf_train.hip (the brute-force index's flat arrays).  The arithmetic is the CPU builder's (rbq_build.cpp), expression
// for expression; -ffp-contract=off.
#pragma once
#include "kernels.hpp"

namespace rbq {

constexpr int kEncTile = 64;             // dims per LDS tile
constexpr int kEncLd = kEncTile + 1;     // row stride (floats): lane i reads word i*65 + k -> conflict-free

// dot8 state: acc[l] += a*b for element index i with l = i % 8 (src/math.rs AVX2 lane order); D % 8 == 0
struct Dot8 {
    float a[8];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int l = 0; l < 8; ++l) a[l] = 0.0f;
    }
    __device__ __forceinline__ float finish(bool any) const {
        float sum = 0.0f;
        if (any) {
            sum = -0.0f;
#pragma unroll
            for (int l = 0; l < 8; ++l) sum = sum + a[l];
        }
        return sum;
    }
};

// SCATTER = false: block-ordered chunk (rbq_index_build_device) — row r IS chunk-local slot r, the 32 lanes of a
//   half-wave share one block and therefore one centroid row.
// SCATTER = true: streamed build (rbq_build_stream_push) — rows are the chunk's vectors sorted by slot, row r goes
//   to GLOBAL slot row_slot[r]; every row stages its own centroid tile.  Same arithmetic, expression for expression.
// OPT = false: RabitqConfig::faster, the constant t_const (widened to f64) for every vector.
// OPT = true: RabitqConfig::new, row r's own best_rescale_factor P.t_row[r] (k_rescale, f64 — never rounded to f32).
// FLAT = true (with SCATTER = false): BruteForceRabitqIndex::train (src/brute_force.rs:214-285) — every row r < nslots is a
//   vector (no slot_src), quantised against the ZERO centroid and written to the brute-force index's flat arrays: sign bytes
//   to P.blocks[r][D/8], the eight factors to P.delta .. P.residual_norm[r].  The zero centroid is staged like any other, so
//   every centroid term stays in its chain (r - 0.0f, the signed zero sums, 0 / INFINITY): nothing is specialised away.
template <bool SCATTER, bool OPT = false, bool FLAT = false>
__global__ __launch_bounds__(kEncThreads) void k_encode(EncodeParams P) {
    static_assert(!(SCATTER && FLAT), "the flat layout is written in row order");
    __shared__ float s_x[kEncThreads * kEncLd];
    __shared__ float s_c[SCATTER ? kEncThreads * kEncLd : 2 * kEncTile];
    const uint32_t tid = threadIdx.x, half = tid >> 5;
    const uint32_t slot = blockIdx.x * kEncThreads + tid;         // row (block-ordered mode: chunk-local slot)
    const uint32_t nblk = (P.nslots + 31u) / 32u;
    const uint32_t src = (slot < P.nslots) ? (FLAT ? slot : P.slot_src[slot]) : kNoSrc;
    const bool valid = src != kNoSrc;
    const uint32_t oslot = SCATTER ? (valid ? P.row_slot[slot] : 0u) : slot; // output slot in the views of P
    const uint32_t blk = SCATTER ? (oslot >> 5) : blockIdx.x * 2 + half;
    const uint32_t v = SCATTER ? (oslot & 31u) : (tid & 31u);
    const bool has_blk = (SCATTER || FLAT) ? valid : blk < nblk;
    const uint32_t D = P.D, Dc = P.Dc, ex_bits = P.ex_bits;
    const size_t stride = (size_t)Dc * 4 + 384;
    uint8_t* rec = P.blocks + (size_t)blk * stride;
    const float F32_EPS = 1.1920929e-07f, K_CONST_EPSILON = 1.9f;

    // coalesced staging of one tile: 64 rows x 256 B, 16 lanes per row; the centroid rows of the two blocks
    auto stage = [&](uint32_t t0) {
        __syncthreads();
        const uint32_t w = D - t0 < (uint32_t)kEncTile ? D - t0 : (uint32_t)kEncTile; // tile width (multiple of 16)
#pragma unroll 4
        for (uint32_t it = 0; it < 16; ++it) {
            const uint32_t r = it * 4 + (tid >> 4), k4 = (tid & 15u) * 4;
            const uint32_t gs = blockIdx.x * kEncThreads + r;
            float4 x = make_float4(0, 0, 0, 0);
            if (gs < P.nslots && k4 < w && (FLAT || P.slot_src[gs] != kNoSrc)) x = *reinterpret_cast<const float4*>(P.rows + (size_t)gs * D + t0 + k4);
            float* d = s_x + r * kEncLd + k4;
            d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
        }
        if (SCATTER) {
#pragma unroll 4
            for (uint32_t it = 0; it < 16; ++it) {
                const uint32_t r = it * 4 + (tid >> 4), k4 = (tid & 15u) * 4;
                const uint32_t gs = blockIdx.x * kEncThreads + r;
                float4 c = make_float4(0, 0, 0, 0);
                if (gs < P.nslots && k4 < w && P.slot_src[gs] != kNoSrc)
                    c = *reinterpret_cast<const float4*>(P.centroids + (size_t)P.block_list[P.row_slot[gs] >> 5] * D + t0 + k4);
                float* d = s_c + r * kEncLd + k4;
                d[0] = c.x; d[1] = c.y; d[2] = c.z; d[3] = c.w;
            }
        } else
        for (uint32_t i = tid; i < 2u * kEncTile; i += kEncThreads) {
            const uint32_t h = i / kEncTile, k = i % kEncTile, b = blockIdx.x * 2 + h;
            s_c[i] = (!FLAT && b < nblk && k < w) ? P.centroids[(size_t)P.block_list[b] * D + t0 + k] : 0.0f;
        }
        __syncthreads();
        return w;
    };

    // ---- pass A: residual, sign bits, |r|^2 chain, the five dots of compute_one_bit_factors
    float n2 = -0.0f;
    Dot8 d_l2, d_xu, d_rx, d_cx, d_rc;
    d_l2.init(); d_xu.init(); d_rx.init(); d_cx.init(); d_rc.init();
    uint32_t gran[4] = {0, 0, 0, 0}; // 16 code bytes (128 dims) being assembled
    for (uint32_t t0 = 0; t0 < D; t0 += kEncTile) {
        const uint32_t w = stage(t0);
        const float* xr = s_x + tid * kEncLd;
        const float* cr = SCATTER ? s_c + tid * kEncLd : s_c + half * kEncTile;
        for (uint32_t k0 = 0; k0 < w; k0 += 8) {
            uint32_t byte = 0;
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                const float c = cr[k0 + l];
                const float r = xr[k0 + l] - c;
                const bool bit = r >= 0.0f;
                byte |= (bit ? 1u : 0u) << (7 - l);
                const float na = fabsf(r);
                { const float p = na * na; n2 = n2 + p; }
                const float xb = (bit ? 1.0f : 0.0f) - 0.5f;
                { const float p = r * r; d_l2.a[l] = d_l2.a[l] + p; }
                { const float p = xb * xb; d_xu.a[l] = d_xu.a[l] + p; }
                { const float p = r * xb; d_rx.a[l] = d_rx.a[l] + p; }
                { const float p = c * xb; d_cx.a[l] = d_cx.a[l] + p; }
                { const float p = r * c; d_rc.a[l] = d_rc.a[l] + p; }
            }
            const uint32_t col = (t0 + k0) >> 3; // byte column of the vector's packed sign code
            gran[(col & 15u) >> 2] |= byte << (8 * (col & 3u));
            if ((col & 15u) == 15u || t0 + k0 + 8 == D) { // granule complete (or the code ends)
                const uint32_t g = col >> 4, G16 = Dc >> 7;
                if (FLAT) { // bin[slot][16 g ..]: the granule's bytes in column order (rows are 2-byte aligned: D % 16 == 0)
                    if (valid) {
                        uint16_t* dst = reinterpret_cast<uint16_t*>(P.blocks + (size_t)slot * (D >> 3) + (size_t)g * 16);
                        const uint32_t nb = (col & 15u) + 1u; // bytes of this granule (even)
                        if ((D & 127u) == 0) *reinterpret_cast<uint4*>(dst) = make_uint4(gran[0], gran[1], gran[2], gran[3]);
                        else {
#pragma unroll
                            for (uint32_t j = 0; j < 8; ++j) // (unrolled: gran stays in registers)
                                if (2 * j < nb) dst[j] = (uint16_t)(gran[j >> 1] >> (16 * (j & 1u)));
                        }
                    }
                } else if (valid) {
                    if (g < G16) *reinterpret_cast<uint4*>(rec + (size_t)g * 512 + v * 16) = make_uint4(gran[0], gran[1], gran[2], gran[3]);
                    else *reinterpret_cast<uint2*>(rec + (size_t)G16 * 512 + v * 8) = make_uint2(gran[0], gran[1]);
                }
                gran[0] = gran[1] = gran[2] = gran[3] = 0;
            }
        }
    }
    const bool any8 = D >= 8;
    const float l2_sqr = d_l2.finish(any8), xu_norm_sqr = d_xu.finish(any8), ip_resi_xucb = d_rx.finish(any8);
    const float ip_cent_xucb = d_cx.finish(any8), dot_res_cent = d_rc.finish(any8);
    const float l2_norm = sqrtf(l2_sqr);
    const float norm = sqrtf(n2);

    // ---- pass B: ex codes (t_const), ipnorm chain in f64, the two dots of compute_extended_factors
    float ipnorm_inv = 1.0f;
    float f_add_ex = 0.0f, f_rescale_ex = 0.0f;
    // reconstruction factors: |u'|^2 and <r, u'> of the centred total code u'.  At ex_bits == 0, u' = bit - 0.5 is pass
    // A's xu_cb, so the two values are xu_norm_sqr and ip_resi_xucb (the same dot8 chains); pass B forms them otherwise.
    float nq2 = xu_norm_sqr, drq = ip_resi_xucb;
    if (ex_bits > 0) { // uniform
        const bool coded = norm > F32_EPS;
        const int32_t max_val = (1 << ex_bits) - 1;
        const double t = OPT ? (valid ? P.t_row[slot] : 0.0) : (double)P.t_const;
        const float cb = -((float)(1u << ex_bits) - 0.5f);
        double ipnorm = 0.0;
        Dot8 d_ipr, d_ipc, d_nq;
        d_ipr.init(); d_ipc.init(); d_nq.init();
        for (uint32_t t0 = 0; t0 < D; t0 += kEncTile) {
            const uint32_t w = stage(t0);
            const float* xr = s_x + tid * kEncLd;
            const float* cr = SCATTER ? s_c + tid * kEncLd : s_c + half * kEncTile;
            for (uint32_t k0 = 0; k0 < w; k0 += 16) {
                uint32_t pk[4] = {0, 0, 0, 0};
#pragma unroll
                for (int l = 0; l < 16; ++l) {
                    const float c = cr[k0 + l];
                    const float r = xr[k0 + l] - c;
                    const bool bit = r >= 0.0f;
                    uint32_t code = 0;
                    if (coded) {
                        const float na = fabsf(r) / norm;
                        int32_t cur = (int32_t)(t * (double)na + 1e-5);
                        if (cur > max_val) cur = max_val;
                        ipnorm += ((double)cur + 0.5) * (double)na;
                        code = (uint32_t)cur;
                        if (r < 0.0f) code = (~code) & (uint32_t)max_val;
                    }
                    const float xu = (float)(uint16_t)(code + ((bit ? 1u : 0u) << ex_bits)) + cb;
                    { const float p = r * xu; d_ipr.a[l & 7] = d_ipr.a[l & 7] + p; }
                    { const float p = c * xu; d_ipc.a[l & 7] = d_ipc.a[l & 7] + p; }
                    if (P.delta) { const float p = xu * xu; d_nq.a[l & 7] = d_nq.a[l & 7] + p; }
                    pk[l >> 2] |= code << (8 * (l & 3));
                }
                if (valid) *reinterpret_cast<uint4*>(P.raw_ex + (size_t)slot * D + t0 + k0) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            }
        }
        if (coded) {
            ipnorm_inv = (isfinite(ipnorm) && ipnorm > 0.0) ? (float)(1.0 / ipnorm) : 1.0f;
            if (!isfinite(ipnorm_inv)) ipnorm_inv = 1.0f;
        }
        const float ip_r = d_ipr.finish(any8), ip_c = d_ipc.finish(any8);
        nq2 = d_nq.finish(any8); drq = ip_r;
        const float safe = fabsf(ip_r) <= F32_EPS ? INFINITY : ip_r;
        if (P.metric == 0) {
            f_add_ex = l2_sqr + 2.0f * l2_sqr * ip_c / safe;
            f_rescale_ex = -2.0f * l2_norm * ipnorm_inv;
        } else {
            f_add_ex = 1.0f - dot_res_cent + l2_sqr * ip_c / safe;
            f_rescale_ex = -l2_norm * ipnorm_inv;
        }
    }

    // ---- compute_one_bit_factors
    float f_add, f_rescale, f_error;
    {
        float denom = ip_resi_xucb;
        if (fabsf(denom) <= F32_EPS) denom = INFINITY;
        float tmp_error = 0.0f;
        if (D > 1) {
            const float ratio = ((l2_sqr * xu_norm_sqr) / (denom * denom)) - 1.0f;
            if (isfinite(ratio) && ratio > 0.0f)
                tmp_error = l2_norm * K_CONST_EPSILON * sqrtf(fmaxf(ratio / (float)(D - 1), 0.0f));
        }
        if (P.metric == 0) {
            f_add = l2_sqr + 2.0f * l2_sqr * ip_cent_xucb / denom;
            f_rescale = -2.0f * l2_sqr / denom;
            f_error = 2.0f * tmp_error;
        } else {
            f_add = 1.0f - dot_res_cent + l2_sqr * ip_cent_xucb / denom;
            f_rescale = -l2_sqr / denom;
            f_error = tmp_error;
        }
    }
    if (has_blk) {
        const uint32_t s = SCATTER ? oslot : FLAT ? slot : blk * 32 + v;
        if (FLAT) {
            P.f_add[s] = f_add; P.f_rescale[s] = f_rescale; P.f_error[s] = f_error;
            P.residual_norm[s] = l2_norm; // fourth output of compute_one_bit_factors (rbq_build.cpp: out.residual_norm)
        } else {
            float* fac = reinterpret_cast<float*>(rec + (size_t)Dc * 4);
            fac[v] = valid ? f_add : 0.0f;
            fac[32 + v] = valid ? f_rescale : 0.0f;
            fac[64 + v] = valid ? f_error : 0.0f;
            P.ids[s] = valid ? P.src_base + src : ~0ull;
        }
        if (ex_bits || FLAT) { // (the flat arrays hold the zeros of a 1-bit index too)
            P.f_add_ex[s] = valid ? f_add_ex : 0.0f;
            P.f_rescale_ex[s] = valid ? f_rescale_ex : 0.0f;
        }
        if (P.delta) { // rbq_build.cpp's delta / vl; std::max / std::min spelt out (NaN passes through as there)
            const float cb = -((float)(1u << ex_bits) - 0.5f);
            const float nq = sqrtf(nq2);
            float den = l2_norm * nq;
            den = den < F32_EPS ? F32_EPS : den;
            float cosv = drq / den;
            cosv = cosv < -1.0f ? -1.0f : cosv;
            cosv = 1.0f < cosv ? 1.0f : cosv;
            const float delta = nq <= F32_EPS ? 0.0f : (l2_norm / nq) * cosv;
            P.delta[s] = valid ? delta : 0.0f;
            P.vl[s] = valid ? delta * cb : 0.0f;
        }
        if (!FLAT && P.residual_norm) P.residual_norm[s] = valid ? l2_norm : 0.0f; // MSTG handles keep it for the `.mstg` format
    }
}

} // namespace rbq
