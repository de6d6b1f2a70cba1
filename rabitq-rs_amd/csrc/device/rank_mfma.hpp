// rank_mfma.hpp — the ranking GEMMs of probe selection through an MFMA shortlist (gfx950), and the derivation of the bound eps that
// the selection behind them (select_mfma.hpp: k_select_mfma) puts on their scores.
//
// Reference: search_fastscan's centroid ranking (src/ivf.rs:1782-1835) with math::l2_distance_sqr / dot in
// their AVX2 lane order (src/math.rs:154-245).  Ranking all nq x nlist pairs in that exact order costs
// 3*nq*nlist*D unfused VALU ops; instead
//   k_rank_bf16_db one split-bf16 MFMA GEMM gives APPROXIMATE scores
//                  A(q,c) = |q|^2 + |c|^2 - 2 q.c   (L2)   or   q.c   (IP)
//                  with x = hi + lo + r (hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-16 |x|) and
//                  q.c ~ qh.ch + qh.cl + ql.ch on v_mfma_f32_32x32x16_bf16 (products exact, f32 accumulate);
//                  the dropped terms are <= 3.01 * 2^-16 * sum|q_i||c_i| <= 1.51 * 2^-16 (|q|^2 + |c|^2)
//   k_rank_mfma    the same scores from one f32 MFMA GEMM (v_mfma_f32_32x32x2_f32), used when D % 64 != 0
//   k_select_mfma  (select_mfma.hpp) per query: nprobe-th approximate score tau, shortlist {c : A(c) within 2*eps of tau},
//                  EXACT canonical-order scores for the shortlist only (canon_score.hpp), exact (score, cid) sort.
// eps bounds |A - canonical| rigorously (standard rounding-error model, n = D, u = 2^-24):
//   |canonical - s*| <= gamma_n s*  (positive terms),  |A - s*| <= 2 gamma_{n+2} (|q|^2 + |c|^2)
//   =>  |A - canonical| <= 4 gamma_{n+2} (|q|^2 + |c|^2)   (s* <= 2(|q|^2+|c|^2));  eps uses 6 n u (..), > that.
// The split-bf16 GEMM accumulates 3n exact products: 2 gamma_{3n+2} * (sum|q_i||c_i| <= (|q|^2+|c|^2)/2) plus the
// norm terms stays below 4 n u (|q|^2+|c|^2) even if the MFMA adder truncates (u -> 2u), and the split itself
// adds 2 * 1.51 * 2^-16 (|q|^2+|c|^2) to the L2 score: eps = (6 n u + 4 * 2^-16)(|q|^2 + max|c|^2).
// Any true top-nprobe member has canonical <= (largest canonical among the approximate top-nprobe) <= tau+eps,
// hence A <= tau + 2 eps: it is in the shortlist.  If the shortlist overflows its LDS capacity (many
// near-equal scores) or a score is not finite, the query falls back to canonical scores for ALL lists.
//
// ONE f16 PRODUCT (k_rank_f16_db; api_search.hip decides per call).  Both operands are rounded once to f16, xh = f16(x) to nearest
// even with every result below 2^-14 stored as a signed zero (types.hpp, f16_rne_flush), and q.c ~ qh.ch on
// v_mfma_f32_32x32x16_f16: n exact products (11 x 11 significant bits, exponents within f32's range) instead of 3n, f32 accumulate.
//   residuals  xl := x - xh is EXACT in f32: a stored normal half lies within a factor 2 of x (Sterbenz), a flushed one is 0 and
//              leaves x itself, so the flush is simply part of xl.  |ql| is measured per query by the preparation kernel, |cl| per
//              centroid when the index is made — squares and sums in f64, roots rounded up — from the bits actually stored.
//              Nothing is assumed about the data's range.
//   split      q.c - qh.ch = ql.c + qh.cl, so |q.c - qh.ch| <= |ql||c| + |qh||cl| (Cauchy-Schwarz), and |qh| <= |q| + |ql|.
//   sum        n products: 2 gamma_{n+2} (sum|qh_i||ch_i| <= (|qh|^2+|ch|^2)/2) plus the norm terms stays below
//              (4/3) n u (|q|^2+|c|^2) (1 + 2^-10)^2 even if the MFMA adder truncates (u -> 2u) — well inside the 4 n u the
//              split-bf16 form already takes of the 6 n u.  No split-K on this route; the + 16 u allowance stays.
//   eps      = ((6 n + 16) u (|q|^2 + max|c|^2) + 2.01 (|ql| max|c| + (|q| + |ql|) max|cl|)) * 1.001
//              (2 x the split term for the L2 score's -2 q.c; .01 and .001: the f32 evaluation of this very expression.)
// The route needs every stored centroid half finite and max|cl| <= 2^-11 max|c| (an index whose centroids lose more than f16's
// relative rounding error to the flush stays on split-bf16); a query whose image is not finite has |ql| and eps not finite and
// takes the fallback.  At D = 960 on unit-scale data eps is about twice the split-bf16 one.
#pragma once
#include "kernels.hpp"

namespace rbq {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// TW = 2: 128x128 tile (64x64 per wave, 4 MFMA per k-pair); TW = 1: 64x64 tile (32x32 per wave) for small
// problems where 128x128 tiles would leave most CUs idle.
template <int METRIC, int TW>
__global__ __launch_bounds__(256) void k_rank_mfma(const float* __restrict__ rot, const float* __restrict__ cent,
                                                   const QueryConsts* __restrict__ consts,
                                                   const float* __restrict__ cnorm2, uint32_t nq, uint32_t nlist,
                                                   uint32_t D, float* __restrict__ scores) {
    constexpr int BM = 64 * TW, BN = 64 * TW, BK = 32, LD = BK + 1; // +1: 32 rows of one k column hit 32 distinct banks
    __shared__ float As[BM][LD];
    __shared__ float Bs[BN][LD];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, wm = w >> 1, wn = w & 1u;
    const uint32_t q0 = blockIdx.y * BM, c0 = blockIdx.x * BN;
    f32x16 acc[TW][TW];
#pragma unroll
    for (int a = 0; a < TW; ++a)
#pragma unroll
        for (int b = 0; b < TW; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    for (uint32_t k0 = 0; k0 < D; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 2 * TW; ++i) { // BM rows x 32 floats = BM*8 float4 per operand
            const uint32_t idx = tid + 256u * i, row = idx >> 3, c4 = (idx & 7u) * 4u, k = k0 + c4;
            float4 av = make_float4(0, 0, 0, 0), bv = make_float4(0, 0, 0, 0);
            if (q0 + row < nq && k < D) av = *reinterpret_cast<const float4*>(rot + (size_t)(q0 + row) * D + k);
            if (c0 + row < nlist && k < D) bv = *reinterpret_cast<const float4*>(cent + (size_t)(c0 + row) * D + k);
            As[row][c4] = av.x; As[row][c4 + 1] = av.y; As[row][c4 + 2] = av.z; As[row][c4 + 3] = av.w;
            Bs[row][c4] = bv.x; Bs[row][c4 + 1] = bv.y; Bs[row][c4 + 2] = bv.z; Bs[row][c4 + 3] = bv.w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const uint32_t r = lane & 31u, kx = kk + (lane >> 5);
            float av[TW], bv[TW];
#pragma unroll
            for (int a = 0; a < TW; ++a) {
                av[a] = As[wm * 32 * TW + a * 32 + r][kx];
                bv[a] = Bs[wn * 32 * TW + a * 32 + r][kx];
            }
#pragma unroll
            for (int a = 0; a < TW; ++a)
#pragma unroll
                for (int b = 0; b < TW; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout of 32x32: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int a = 0; a < TW; ++a)
#pragma unroll
        for (int b = 0; b < TW; ++b) {
            const uint32_t c = c0 + wn * 32 * TW + b * 32 + (lane & 31u);
            const float cn = (METRIC == 0 && c < nlist) ? cnorm2[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t qi = q0 + wm * 32 * TW + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (qi < nq && c < nlist) {
                    const float dot = acc[a][b][r];
                    float v = dot;
                    if (METRIC == 0) {
                        const float qn = consts[qi].qnorm2;
                        v = fmaf(-2.0f, dot, qn + cn);
                    }
                    scores[(size_t)qi * nlist + c] = v;
                }
            }
        }
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma_x8(bf16x8 a, bf16x8 b, f32x16 c) { // one K = 16 step: c += a(32x16) * b(16x32)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); // gfx950's double-rate form
}

// Split-bf16 GEMM (32*TM*WM x 32*TN*WN tile per workgroup of WM*WN wavefronts, each wavefront a 32*TM x 32*TN
// sub-tile of 32x32 MFMA blocks) with K slabs of 32 double-buffered in LDS: slab s+1 is written (from the registers
// the previous iteration filled) and slab s+2 requested BEFORE the MFMAs of slab s, and one barrier per slab closes
// the iteration — the staging of the next slab runs under the matrix work of this one instead of between two
// barriers.
// Rows are padded to 80 bytes (16 lanes of a ds_read_b128 group: 16 distinct 4-bank sets).  D % 32 == 0.
// dynamic LDS: 2 x { Ah | Al [BM][80 B] | Bh | Bl [BN][80 B] }
// OPERANDS.  Each of A (queries) and B (centroids) comes as the bases of its hi and lo planes, a row stride and a K-slab stride, in bytes:
//   planar      two arrays [rows][D] bf16: row stride 2 D, slab stride 64.  Four consecutive lanes fetch the 64 bytes of one row and
//               plane, so a wave-level 16-byte load touches 16 lines of 128 bytes and uses half of each; the other half is the NEXT
//               slab's, by which time the workgroup has pulled a whole slab of both operands through the vector L1.
//   interleaved ONE array [rows][2 D] (hl_layout.hpp: slab s of a row = 128 bytes, hi | lo): the lo base is 64 bytes behind the
//               hi base, row stride 4 D, slab stride 128 — what selects this lane map.  A wave-level load then covers 8 rows x 128
//               bytes, whole lines: lanes 0..31 the hi halves of rows r..r+7 (4 lanes per row), lanes 32..63 their lo halves, and a
//               thread's second load of a pair is 8 rows further on instead of in the other plane.  Within a plane the rows go
//               0, 4, 1, 5, 2, 6, 3, 7: a ds_write_b128 is served in groups of 8 lanes over 32 banks, and with rows of 80 bytes (20
//               banks) rows r and r + 4 are 16 banks apart — no conflict, where the planar map's r and r + 1 share four banks.
// Same number of loads per thread either way, and the LDS images — hence fragments, MFMA order and scores — are byte for byte the same.
template <int METRIC, int TM, int TN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void k_rank_bf16_db(const unsigned char* __restrict__ a_hi, const unsigned char* __restrict__ a_lo,
                                                      uint32_t a_row, uint32_t a_slab,
                                                      const unsigned char* __restrict__ b_hi, const unsigned char* __restrict__ b_lo,
                                                      uint32_t b_row, uint32_t b_slab,
                                                      const QueryConsts* __restrict__ consts,
                                                      const float* __restrict__ cnorm2, uint32_t nq, uint32_t nlist,
                                                      uint32_t D, float* __restrict__ scores) {
    constexpr int NT = 64 * WM * WN, BM = 32 * TM * WM, BN = 32 * TN * WN, BK = 32, LDB = BK * 2 + 16, SEG = BK / 8;
    constexpr int NLA = BM * SEG / NT, NLB = BN * SEG / NT; // 16-byte loads per thread and array
    constexpr int BUF = (2 * BM + 2 * BN) * LDB;
    static_assert(BM * SEG % NT == 0 && BN * SEG % NT == 0, "tile rows must divide over the threads");
    extern __shared__ __align__(16) unsigned char smraw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, wm = w / WN, wn = w % WN;
    const uint32_t q0 = blockIdx.y * BM, c0 = blockIdx.x * BN;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
    static_assert(BM % 16 == 0 && BN % 16 == 0, "the interleaved lane map takes 16 rows per wave-level pair of loads");
    // pair i of a thread's loads: ga_h / ga_l (gb_h / gb_l) are its two addresses, soa (sob) the LDS offset of the first and soa + dla
    // (sob + dlb) that of the second — planar: (row, hi) and (row, lo); interleaved: (row, plane) and (row + 8, plane)
    const unsigned char* ga_h[NLA];
    const unsigned char* ga_l[NLA];
    const unsigned char* gb_h[NLB];
    const unsigned char* gb_l[NLB];
    uint32_t soa[NLA], sob[NLB];
    const bool a_il = a_slab == 4u * BK, b_il = b_slab == 4u * BK; // (uniform)
    const uint32_t dla = a_il ? 8u * LDB : (uint32_t)BM * LDB, dlb = b_il ? 8u * LDB : (uint32_t)BN * LDB;
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
        const uint32_t idx = tid + (uint32_t)NT * i;
        if (a_il) {
            const uint32_t q4 = (idx & 31u) >> 2, row = (idx >> 6) * 16u + ((q4 & 1u) << 2 | q4 >> 1), plane = (idx >> 5) & 1u, seg = idx & 3u;
            const uint32_t r0 = q0 + row < nq ? q0 + row : nq - 1u, r1 = q0 + row + 8u < nq ? q0 + row + 8u : nq - 1u;
            const unsigned char* pb = (plane ? a_lo : a_hi) + seg * 16;
            ga_h[i] = pb + (size_t)r0 * a_row;
            ga_l[i] = pb + (size_t)r1 * a_row;
            soa[i] = plane * BM * LDB + row * LDB + seg * 16;
        } else {
            const uint32_t row = idx / SEG, seg = idx % SEG;
            const uint32_t ra = q0 + row < nq ? q0 + row : nq - 1u;
            ga_h[i] = a_hi + (size_t)ra * a_row + seg * 16;
            ga_l[i] = a_lo + (size_t)ra * a_row + seg * 16;
            soa[i] = row * LDB + seg * 16;
        }
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
        const uint32_t idx = tid + (uint32_t)NT * i;
        if (b_il) {
            const uint32_t q4 = (idx & 31u) >> 2, row = (idx >> 6) * 16u + ((q4 & 1u) << 2 | q4 >> 1), plane = (idx >> 5) & 1u, seg = idx & 3u;
            const uint32_t r0 = c0 + row < nlist ? c0 + row : nlist - 1u, r1 = c0 + row + 8u < nlist ? c0 + row + 8u : nlist - 1u;
            const unsigned char* pb = (plane ? b_lo : b_hi) + seg * 16;
            gb_h[i] = pb + (size_t)r0 * b_row;
            gb_l[i] = pb + (size_t)r1 * b_row;
            sob[i] = 2 * BM * LDB + plane * BN * LDB + row * LDB + seg * 16;
        } else {
            const uint32_t row = idx / SEG, seg = idx % SEG;
            const uint32_t rb = c0 + row < nlist ? c0 + row : nlist - 1u;
            gb_h[i] = b_hi + (size_t)rb * b_row + seg * 16;
            gb_l[i] = b_lo + (size_t)rb * b_row + seg * 16;
            sob[i] = 2 * BM * LDB + row * LDB + seg * 16;
        }
    }
    u32x4 pah[NLA], pal[NLA], pbh[NLB], pbl[NLB];
    // SPLIT-K (gridDim.z > 1; small batches, whose few tiles leave most of the chip idle while each walks all D / 32 slabs): workgroup z
    // takes the slabs [z * per, (z + 1) * per) and ADDS its part of the score atomically to a row the preparation kernel zeroed
    // (z = 0 also adds the norms).  The order of those additions is not fixed; the approximate score only feeds the shortlist, whose
    // eps covers it (k_select_mfma), and every result is decided on exact scores.
    const uint32_t nslab_all = D / BK, per_z = (nslab_all + gridDim.z - 1u) / gridDim.z, s_first = blockIdx.z * per_z;
    if (s_first >= nslab_all) return; // (whole workgroup)
    const uint32_t nslab = nslab_all - s_first < per_z ? nslab_all - s_first : per_z;
    {
        const size_t ka_first = (size_t)s_first * a_slab, kb_first = (size_t)s_first * b_slab;
#pragma unroll
        for (int i = 0; i < NLA; ++i) { ga_h[i] += ka_first; ga_l[i] += ka_first; }
#pragma unroll
        for (int i = 0; i < NLB; ++i) { gb_h[i] += kb_first; gb_l[i] += kb_first; }
    }
#define RBQ_RANK_FETCH(S)                                                                                              \
    do {                                                                                                               \
        const size_t koa = (size_t)(S) * a_slab, kob = (size_t)(S) * b_slab;                                           \
        _Pragma("unroll") for (int i = 0; i < NLA; ++i) {                                                              \
            pah[i] = *reinterpret_cast<const u32x4*>(ga_h[i] + koa);                                                   \
            pal[i] = *reinterpret_cast<const u32x4*>(ga_l[i] + koa);                                                   \
        }                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < NLB; ++i) {                                                              \
            pbh[i] = *reinterpret_cast<const u32x4*>(gb_h[i] + kob);                                                   \
            pbl[i] = *reinterpret_cast<const u32x4*>(gb_l[i] + kob);                                                   \
        }                                                                                                              \
    } while (0)
#define RBQ_RANK_STORE(B)                                                                                              \
    do {                                                                                                               \
        unsigned char* base = smraw + (B) * BUF;                                                                       \
        _Pragma("unroll") for (int i = 0; i < NLA; ++i) {                                                              \
            *reinterpret_cast<u32x4*>(base + soa[i]) = pah[i];                                                         \
            *reinterpret_cast<u32x4*>(base + dla + soa[i]) = pal[i];                                                   \
        }                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < NLB; ++i) {                                                              \
            *reinterpret_cast<u32x4*>(base + sob[i]) = pbh[i];                                                         \
            *reinterpret_cast<u32x4*>(base + dlb + sob[i]) = pbl[i];                                                   \
        }                                                                                                              \
    } while (0)
    // fragment sets of the two 16-wide K steps of a slab; A/B operand of the MFMA: lane l holds row (l & 31),
    // k = 8 * (l >> 5) .. + 7
    bf16x8 f0ah[TM], f0al[TM], f0bh[TN], f0bl[TN], f1ah[TM], f1al[TM], f1bh[TN], f1bl[TN];
    const uint32_t fo = (lane & 31u) * LDB + (lane >> 5) * 16;
#define RBQ_RANK_FRAGS(B, KC, AH, AL, BH, BL)                                                                          \
    do {                                                                                                               \
        const unsigned char* sAh = smraw + (B) * BUF;                                                                  \
        const unsigned char* sBh = sAh + 2 * BM * LDB;                                                                 \
        _Pragma("unroll") for (int a = 0; a < TM; ++a) {                                                               \
            const uint32_t ra = (wm * 32 * TM + a * 32) * LDB + fo + (KC) * 32;                                        \
            AH[a] = *reinterpret_cast<const bf16x8*>(sAh + ra);                                                        \
            AL[a] = *reinterpret_cast<const bf16x8*>(sAh + BM * LDB + ra);                                             \
        }                                                                                                              \
        _Pragma("unroll") for (int b = 0; b < TN; ++b) {                                                               \
            const uint32_t rb = (wn * 32 * TN + b * 32) * LDB + fo + (KC) * 32;                                        \
            BH[b] = *reinterpret_cast<const bf16x8*>(sBh + rb);                                                        \
            BL[b] = *reinterpret_cast<const bf16x8*>(sBh + BN * LDB + rb);                                             \
        }                                                                                                              \
    } while (0)
    // The MFMA is gfx950's double-rate v_mfma_f32_32x32x16_bf16 (mfma_x8 above).  Round 1 had seen wrong LUT bytes from
    // the workgroup-per-query k_prep of a NEIGHBOURING stream while an x16 MFMA GEMM ran — in the single-buffered GEMM
    // kernel of that time, which no longer exists.  With this kernel the combination was re-examined in round 2
    // (tests/diag/x16_probe.py, x16_tests.py: 3000 rounds of a k_prep victim stream beside three noise streams compared
    // byte for byte with a quiet run, 12 rounds of the two multi-stream parity tests with k_prep forced): no difference,
    // so the interaction went with the kernel it was seen in.  test_concurrent_streams_match_oracle (both preparation
    // kernels) and test_matrix_rotator_concurrent_streams guard the multi-stream path.  (The K = 8 form kept behind a switch until then is gone.)
#define RBQ_RANK_MMA(AH, AL, BH, BL)                                                                                   \
    _Pragma("unroll") for (int a = 0; a < TM; ++a) _Pragma("unroll") for (int b = 0; b < TN; ++b) {                    \
        acc[a][b] = mfma_x8(AL[a], BH[b], acc[a][b]);                                                                  \
        acc[a][b] = mfma_x8(AH[a], BL[b], acc[a][b]);                                                                  \
        acc[a][b] = mfma_x8(AH[a], BH[b], acc[a][b]);                                                                  \
    }
    RBQ_RANK_FETCH(0);
    RBQ_RANK_STORE(0);
    if (nslab > 1) RBQ_RANK_FETCH(1);
    __syncthreads();
    RBQ_RANK_FRAGS(0, 0, f0ah, f0al, f0bh, f0bl);
    for (uint32_t s = 0; s < nslab; ++s) {
        // the LDS reads of one K step run under the MFMAs of the other: step 1 of this slab is requested before
        // the MFMAs of step 0, step 0 of the NEXT slab (complete in LDS once the barrier is passed) before those
        // of step 1
        const uint32_t cur = s & 1u;
        RBQ_RANK_FRAGS(cur, 1, f1ah, f1al, f1bh, f1bl);
        if (s + 1 < nslab) RBQ_RANK_STORE(cur ^ 1u);
        if (s + 2 < nslab) RBQ_RANK_FETCH(s + 2);
        RBQ_RANK_MMA(f0ah, f0al, f0bh, f0bl);
        __builtin_amdgcn_sched_barrier(0); // keep these MFMAs in front of the barrier: they cover the reads of step 1
        __syncthreads();
        if (s + 1 < nslab) RBQ_RANK_FRAGS(cur ^ 1u, 0, f0ah, f0al, f0bh, f0bl);
        RBQ_RANK_MMA(f1ah, f1al, f1bh, f1bl);
    }
#undef RBQ_RANK_FRAGS
#undef RBQ_RANK_MMA
#undef RBQ_RANK_FETCH
#undef RBQ_RANK_STORE
    // C/D layout of 32x32: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  The query norms of
    // all rows are fetched up front (one wait instead of one per row).
    float qn[TM][16];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t qi = q0 + wm * 32 * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            qn[a][r] = METRIC == 0 ? consts[qi < nq ? qi : nq - 1u].qnorm2 : 0.0f;
        }
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const uint32_t c = c0 + wn * 32 * TN + b * 32 + (lane & 31u);
            const float cn = (METRIC == 0 && c < nlist) ? cnorm2[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t qi = q0 + wm * 32 * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (qi < nq && c < nlist) {
                    const float dot = acc[a][b][r];
                    if (gridDim.z == 1) scores[(size_t)qi * nlist + c] = METRIC == 0 ? fmaf(-2.0f, dot, qn[a][r] + cn) : dot;
                    else atomicAdd(&scores[(size_t)qi * nlist + c], METRIC == 0 ? (blockIdx.z == 0 ? fmaf(-2.0f, dot, qn[a][r] + cn) : -2.0f * dot) : dot);
                }
            }
        }
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// One-product f16 GEMM (header: "ONE f16 PRODUCT"): the structure of k_rank_bf16_db — same tiles, double-buffered LDS, one barrier per
// slab, same epilogue — on ONE image per operand, [rows][D] f16, with K slabs of 64: a slab of a row is one aligned 128-byte line.
//   loads  eight consecutive lanes fetch the eight 16-byte segments of one row's line, so a wave-level load covers 8 rows x 128 bytes,
//          whole lines, and the same eight lanes store them with one ds_write_b128 group: 128 consecutive bytes, 32 distinct banks.
//   LDS    rows of 144 bytes (128 + 16): 9 slots of 16 bytes, odd, so the 16 rows of a ds_read_b128 lane group ({0-3, 12-15, 20-27}
//          and its likes: 16 distinct residues mod 16) fall on 16 distinct 4-bank sets of the 64 banks — conflict-free.
//          dynamic LDS: 2 x { A [BM][144 B] | B [BN][144 B] }
//   K loop four 16-wide steps per slab on two alternating fragment sets: the LDS reads of step k + 1 are requested before the MFMAs of
//          step k; the next slab's step 0 is read behind the barrier, under the MFMAs of this slab's step 3.
// No split-K (gridDim.z == 1).  D % 64 == 0.
template <int METRIC, int TM, int TN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void k_rank_f16_db(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                     const QueryConsts* __restrict__ consts, const float* __restrict__ cnorm2,
                                                     uint32_t nq, uint32_t nlist, uint32_t D, float* __restrict__ scores) {
    constexpr int NT = 64 * WM * WN, BM = 32 * TM * WM, BN = 32 * TN * WN, BK = 64, LDB = BK * 2 + 16, SEG = BK / 8;
    constexpr int NLA = BM * SEG / NT, NLB = BN * SEG / NT; // 16-byte loads per thread and operand
    constexpr int BUF = (BM + BN) * LDB;
    static_assert(BM * SEG % NT == 0 && BN * SEG % NT == 0, "tile rows must divide over the threads");
    extern __shared__ __align__(16) unsigned char smraw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, wm = w / WN, wn = w % WN;
    const uint32_t q0 = blockIdx.y * BM, c0 = blockIdx.x * BN;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int x = 0; x < TM; ++x)
#pragma unroll
        for (int y = 0; y < TN; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
    const unsigned char* ga[NLA];
    const unsigned char* gb[NLB];
    uint32_t soa[NLA], sob[NLB];
    const size_t row_bytes = (size_t)D * 2;
#pragma unroll
    for (int i = 0; i < NLA; ++i) { // (rows past the end re-read the last row: their scores are never stored)
        const uint32_t idx = tid + (uint32_t)NT * i, row = idx / SEG, seg = idx % SEG;
        const uint32_t ra = q0 + row < nq ? q0 + row : nq - 1u;
        ga[i] = a + (size_t)ra * row_bytes + seg * 16;
        soa[i] = row * LDB + seg * 16;
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
        const uint32_t idx = tid + (uint32_t)NT * i, row = idx / SEG, seg = idx % SEG;
        const uint32_t rb = c0 + row < nlist ? c0 + row : nlist - 1u;
        gb[i] = b + (size_t)rb * row_bytes + seg * 16;
        sob[i] = BM * LDB + row * LDB + seg * 16;
    }
    u32x4 pa[NLA], pb[NLB];
    const uint32_t nslab = D / BK;
#define RBQ_RANK_FETCH(S)                                                                                              \
    do {                                                                                                               \
        const size_t ko = (size_t)(S) * (BK * 2);                                                                      \
        _Pragma("unroll") for (int i = 0; i < NLA; ++i) pa[i] = *reinterpret_cast<const u32x4*>(ga[i] + ko);           \
        _Pragma("unroll") for (int i = 0; i < NLB; ++i) pb[i] = *reinterpret_cast<const u32x4*>(gb[i] + ko);           \
    } while (0)
#define RBQ_RANK_STORE(B)                                                                                              \
    do {                                                                                                               \
        unsigned char* base = smraw + (B) * BUF;                                                                       \
        _Pragma("unroll") for (int i = 0; i < NLA; ++i) *reinterpret_cast<u32x4*>(base + soa[i]) = pa[i];              \
        _Pragma("unroll") for (int i = 0; i < NLB; ++i) *reinterpret_cast<u32x4*>(base + sob[i]) = pb[i];              \
    } while (0)
    // A/B operand of v_mfma_f32_32x32x16_f16: lane l holds row (l & 31), k = 8 * (l >> 5) .. + 7 of the 16-wide step
    f16x8 f0a[TM], f0b[TN], f1a[TM], f1b[TN];
    const uint32_t fo = (lane & 31u) * LDB + (lane >> 5) * 16;
#define RBQ_RANK_FRAGS(B, KC, FA, FB)                                                                                  \
    do {                                                                                                               \
        const unsigned char* sA = smraw + (B) * BUF;                                                                   \
        const unsigned char* sB = sA + BM * LDB;                                                                       \
        _Pragma("unroll") for (int x = 0; x < TM; ++x)                                                                 \
            FA[x] = *reinterpret_cast<const f16x8*>(sA + (wm * 32 * TM + x * 32) * LDB + fo + (KC) * 32);              \
        _Pragma("unroll") for (int y = 0; y < TN; ++y)                                                                 \
            FB[y] = *reinterpret_cast<const f16x8*>(sB + (wn * 32 * TN + y * 32) * LDB + fo + (KC) * 32);              \
    } while (0)
#define RBQ_RANK_MMA(FA, FB)                                                                                           \
    _Pragma("unroll") for (int x = 0; x < TM; ++x) _Pragma("unroll") for (int y = 0; y < TN; ++y)                      \
        acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_f16(FA[x], FB[y], acc[x][y], 0, 0, 0);
    RBQ_RANK_FETCH(0);
    RBQ_RANK_STORE(0);
    if (nslab > 1) RBQ_RANK_FETCH(1);
    __syncthreads();
    RBQ_RANK_FRAGS(0, 0, f0a, f0b);
    for (uint32_t s = 0; s < nslab; ++s) {
        const uint32_t cur = s & 1u;
        RBQ_RANK_FRAGS(cur, 1, f1a, f1b);
        if (s + 1 < nslab) RBQ_RANK_STORE(cur ^ 1u); // (that buffer's last reads were waited for in front of the previous barrier)
        if (s + 2 < nslab) RBQ_RANK_FETCH(s + 2);
        RBQ_RANK_MMA(f0a, f0b);
        RBQ_RANK_FRAGS(cur, 2, f0a, f0b);
        RBQ_RANK_MMA(f1a, f1b);
        RBQ_RANK_FRAGS(cur, 3, f1a, f1b);
        RBQ_RANK_MMA(f0a, f0b);
        __builtin_amdgcn_sched_barrier(0); // keep these MFMAs in front of the barrier: they cover the reads of step 3
        __syncthreads();
        if (s + 1 < nslab) RBQ_RANK_FRAGS(cur ^ 1u, 0, f0a, f0b);
        RBQ_RANK_MMA(f1a, f1b);
    }
#undef RBQ_RANK_FRAGS
#undef RBQ_RANK_MMA
#undef RBQ_RANK_FETCH
#undef RBQ_RANK_STORE
    // the epilogue of k_rank_bf16_db without its split-K branch
    float qn[TM][16];
#pragma unroll
    for (int x = 0; x < TM; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t qi = q0 + wm * 32 * TM + x * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            qn[x][r] = METRIC == 0 ? consts[qi < nq ? qi : nq - 1u].qnorm2 : 0.0f;
        }
#pragma unroll
    for (int x = 0; x < TM; ++x)
#pragma unroll
        for (int y = 0; y < TN; ++y) {
            const uint32_t c = c0 + wn * 32 * TN + y * 32 + (lane & 31u);
            const float cn = (METRIC == 0 && c < nlist) ? cnorm2[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t qi = q0 + wm * 32 * TM + x * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (qi < nq && c < nlist) scores[(size_t)qi * nlist + c] = METRIC == 0 ? fmaf(-2.0f, acc[x][y][r], qn[x][r] + cn) : acc[x][y][r];
            }
        }
}

} // namespace rbq
