// k_rescale.hip — best_rescale_factor (src/quantizer.rs:337-427) of every vector on the GPU: the per-vector rescale
// factor t of RabitqConfig::new, which k_encode<*, true> then uses in place of the constant t_const.  gfx950 only.
//
// One workgroup per vector.  The crate sweeps a min-heap of events (t = k / o_i, coordinate i) in ascending (t, i)
// order; the sweep restated:
//   * the events of coordinate i are k = c_i + 1 .. K_i, a contiguous run (k / o_i is monotone in k): the first one
//     whatever its k, the later ones while k <= 2^ex - 1, all of them only while t < t_end;
//   * sqr_den (a multiple of 0.25 far below 2^53) is an exact integer prefix sum — kept as 4 * sqr_den in u64;
//   * num += o_i rounds, so it is ONE sequential f64 chain in event order (one lane walks it);
//   * ip = num / sqrt(sqr_den) per event is independent once num is known: computed by the whole workgroup;
//   * the result is the t of the first event with the largest ip (ties -> lower position in the sorted order).
// The events are generated into LDS in t-windows [T_prev, T): every event with t < T that has not been swept yet.
// A window holds at most kResCap events; a window that would hold more is halved (events of one coordinate lie >= 1
// apart in t because o_i <= 1, so a window narrower than 1/2 holds at most D <= 2048 events and the halving ends).
// Each window is bitonic-sorted on (t bits, coordinate) — t > 0, so the f64 bit pattern orders like the value — and
// swept.  No private arrays: every per-coordinate state lives in LDS, so the kernel uses no scratch.
#include <hip/hip_runtime.h>
#include <cfloat>

#include "launch.hpp"

namespace rbq {
namespace {

constexpr uint32_t kResThreads = 256;
constexpr uint32_t kResCap = 4096;  // events per window (a power of two: the bitonic network's size)
constexpr uint32_t kResMaxD = 2048;

__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* s, uint32_t tid, uint32_t& total) {
    s[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kResThreads; off <<= 1) {
        const uint32_t a = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    const uint32_t incl = s[tid];
    total = s[kResThreads - 1];
    __syncthreads();
    return incl - v;
}

} // namespace

// rows [nrows][D]: rotated vectors (raw_o = 0: o = |row - centroid| / norm) or o itself (raw_o = 1, test hook).
// t[r] = best_rescale_factor; 0 for a vector whose residual norm is <= FLT_EPSILON (k_encode forms no ex code for it).
__global__ __launch_bounds__(kResThreads) void k_rescale(const float* __restrict__ rows, const float* __restrict__ centroids,
                                                         const uint32_t* __restrict__ block_list, const uint32_t* __restrict__ row_slot,
                                                         const uint32_t* __restrict__ slot_src, uint32_t D, uint32_t ex_bits,
                                                         int raw_o, double* __restrict__ t_out) {
    __shared__ uint64_t s_key[kResCap];  // t bits of an event; after the sweep: num after that event (f64 bits)
    __shared__ uint32_t s_pay[kResCap];  // coordinate << 8 | k
    __shared__ float s_o[kResMaxD];
    __shared__ uint16_t s_next[kResMaxD], s_cap[kResMaxD]; // next k of a coordinate, last k it may take
    __shared__ uint32_t s_scan[kResThreads], s_j[kResThreads];
    __shared__ double s_ip[kResThreads];
    __shared__ float s_f[kResThreads];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    if (slot_src && slot_src[r] == kNoSrc) return; // uniform
    const float F32_EPS = 1.1920929e-07f;
    const float* x = rows + (size_t)r * D;

    // ---- o = |r_i| / norm, norm the sequential f32 chain of k_encode's pass A
    if (raw_o) {
        for (uint32_t i = tid; i < D; i += kResThreads) s_o[i] = x[i];
        __syncthreads();
    } else {
        const float* c = centroids + (size_t)block_list[(row_slot ? row_slot[r] : r) >> 5] * D;
        for (uint32_t i = tid; i < D; i += kResThreads) s_o[i] = fabsf(x[i] - c[i]);
        __syncthreads();
        if (tid == 0) {
            float n2 = -0.0f;
            for (uint32_t i = 0; i < D; ++i) { const float p = s_o[i] * s_o[i]; n2 = n2 + p; }
            s_f[0] = sqrtf(n2);
        }
        __syncthreads();
        const float norm = s_f[0];
        if (!(norm > F32_EPS)) { // uniform
            if (tid == 0) t_out[r] = 0.0;
            return;
        }
        __syncthreads();
        for (uint32_t i = tid; i < D; i += kResThreads) s_o[i] = s_o[i] / norm;
        __syncthreads();
    }

    // ---- max_o, t_end, t_start
    float mx = 0.0f;
    for (uint32_t i = tid; i < D; i += kResThreads) mx = fmaxf(mx, s_o[i]);
    s_f[tid] = mx;
    __syncthreads();
    for (uint32_t h = kResThreads / 2; h > 0; h >>= 1) {
        if (tid < h) s_f[tid] = fmaxf(s_f[tid], s_f[tid + h]);
        __syncthreads();
    }
    const double max_o = (double)s_f[0];
    if (max_o <= DBL_EPSILON) { // uniform
        if (tid == 0) t_out[r] = 1.0;
        return;
    }
    // K_TIGHT_START[ex] (src/quantizer.rs), selected without a private array (no scratch)
    const double tight = ex_bits == 1 ? 0.15 : ex_bits == 2 ? 0.20 : ex_bits == 3 ? 0.52 : ex_bits == 4 ? 0.59
                       : ex_bits == 5 ? 0.71 : ex_bits == 6 ? 0.75 : 0.77;
    const int32_t max_val = (1 << ex_bits) - 1;
    const double t_end = ((double)max_val + 10.0) / max_o;
    const double t_start = t_end * tight;

    // ---- start codes; 4 * sqr_den0 = D + 4 sum(c^2 + c) (exact)
    uint32_t sq_part = 0;
    for (uint32_t i = tid; i < D; i += kResThreads) {
        const float o = s_o[i];
        const int32_t c = (int32_t)(t_start * (double)o + 1e-5);
        s_next[i] = (uint16_t)(c + 1);
        s_cap[i] = o > 0.0f ? (uint16_t)(c + 1 > max_val ? c + 1 : max_val) : (uint16_t)0;
        sq_part += (uint32_t)(c * c + c);
    }
    uint32_t sq_tot;
    (void)block_scan_excl(sq_part, s_scan, tid, sq_tot);
    uint64_t sq4 = (uint64_t)D + 4ull * sq_tot;
    // num0 = sum ((double)c_i + 0.5) * (double)o_i, rounded: in index order
    double num = 0.0; // lane 0 only
    if (tid == 0)
        for (uint32_t i = 0; i < D; ++i) num += ((double)((int32_t)s_next[i] - 1) + 0.5) * (double)s_o[i];

    double max_ip = 0.0, best_t = t_start; // uniform
    double T_prev = t_start, w = t_end - t_start + 1.0;
    for (;;) {
        const double T = T_prev + w >= t_end ? t_end : T_prev + w;
        uint32_t mine = 0;
        for (uint32_t i = tid; i < D; i += kResThreads) {
            const double od = (double)s_o[i];
            for (uint32_t k = s_next[i], cap = s_cap[i]; k <= cap && (double)k / od < T; ++k) ++mine;
        }
        uint32_t n;
        uint32_t pos = block_scan_excl(mine, s_scan, tid, n);
        if (n > kResCap) { w *= 0.5; continue; } // uniform
        if (n) {
            // generate, sort
            for (uint32_t i = tid; i < D; i += kResThreads) {
                const double od = (double)s_o[i];
                uint32_t k = s_next[i];
                for (const uint32_t cap = s_cap[i]; k <= cap; ++k) {
                    const double t = (double)k / od;
                    if (!(t < T)) break;
                    s_key[pos] = (uint64_t)__double_as_longlong(t);
                    s_pay[pos] = (i << 8) | k;
                    ++pos;
                }
                s_next[i] = (uint16_t)k;
            }
            uint32_t npad = 2;
            while (npad < n) npad <<= 1;
            for (uint32_t j = n + tid; j < npad; j += kResThreads) { s_key[j] = ~0ull; s_pay[j] = ~0u; }
            __syncthreads();
            for (uint32_t k = 2; k <= npad; k <<= 1)
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t p = tid; p < npad / 2; p += kResThreads) {
                        const uint32_t a = ((p & ~(j - 1)) << 1) | (p & (j - 1)), b = a | j;
                        const uint64_t ka = s_key[a], kb = s_key[b];
                        const uint32_t pa = s_pay[a], pb = s_pay[b];
                        const bool gt = ka > kb || (ka == kb && pa > pb);
                        if (gt == ((a & k) == 0)) { s_key[a] = kb; s_key[b] = ka; s_pay[a] = pb; s_pay[b] = pa; }
                    }
                    __syncthreads();
                }
            // the num chain, in event order
            if (tid == 0) {
                for (uint32_t j = 0; j < n; ++j) {
                    num += (double)s_o[s_pay[j] >> 8];
                    s_key[j] = (uint64_t)__double_as_longlong(num);
                }
            }
            __syncthreads();
            // sqr_den after every event (exact prefix sums over contiguous ranges), ip, first maximum
            const uint32_t per = (n + kResThreads - 1) / kResThreads, j0 = tid * per < n ? tid * per : n,
                           j1 = j0 + per < n ? j0 + per : n;
            uint32_t s8 = 0;
            for (uint32_t j = j0; j < j1; ++j) s8 += 8u * (s_pay[j] & 255u);
            uint32_t s8_tot;
            uint64_t sq = sq4 + block_scan_excl(s8, s_scan, tid, s8_tot);
            double bip = -1.0;
            uint32_t bj = ~0u;
            for (uint32_t j = j0; j < j1; ++j) {
                sq += 8u * (s_pay[j] & 255u);
                const double ip = __longlong_as_double((long long)s_key[j]) / sqrt((double)sq * 0.25);
                if (ip > bip) { bip = ip; bj = j; }
            }
            s_ip[tid] = bip; s_j[tid] = bj;
            __syncthreads();
            for (uint32_t h = kResThreads / 2; h > 0; h >>= 1) {
                if (tid < h) {
                    const double o_ip = s_ip[tid + h];
                    const uint32_t o_j = s_j[tid + h];
                    if (o_ip > s_ip[tid] || (o_ip == s_ip[tid] && o_j < s_j[tid])) { s_ip[tid] = o_ip; s_j[tid] = o_j; }
                }
                __syncthreads();
            }
            if (s_ip[0] > max_ip) { // uniform
                const uint32_t pj = s_pay[s_j[0]];
                max_ip = s_ip[0];
                best_t = (double)(pj & 255u) / (double)s_o[pj >> 8];
            }
            sq4 += s8_tot;
            __syncthreads();
        }
        if (T == t_end) break;
        T_prev = T;
        if (n < kResCap / 2) w *= 2.0;
    }
    if (tid == 0) t_out[r] = best_t <= 0.0 ? fmax(t_start, DBL_EPSILON) : best_t;
}

hipError_t launch_rescale(const float* rows, const float* centroids, const uint32_t* block_list, const uint32_t* row_slot,
                          const uint32_t* slot_src, uint32_t nrows, uint32_t D, uint32_t ex_bits, bool raw_o, double* t,
                          hipStream_t s) {
    if (!nrows) return hipSuccess;
    if (D == 0 || D > kResMaxD || ex_bits == 0 || ex_bits > 7) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rescale, dim3(nrows), dim3(kResThreads), 0, s, rows, centroids, block_list, row_slot, slot_src, D, ex_bits,
                       raw_o ? 1 : 0, t);
    return hipGetLastError();
}

} // namespace rbq
