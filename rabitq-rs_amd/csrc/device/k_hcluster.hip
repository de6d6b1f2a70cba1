// k_hcluster.hip — MSTG step 1 on the device: HierarchicalClustering::cluster (reference src/mstg/clustering.rs) in the pinned
// arithmetic of the CPU restatement rbq_build_hcluster (csrc/host/rbq_hcluster.hpp), which this unit reproduces bit for bit.
// gfx950 only.
//
// Clusters are segments of one device array of row indices (`members`); the rows themselves are never copied per level, only
// gathered once per split into a scratch image sized for the root.  Every buffer is allocated once, for the root.  A split:
//   k_hc_gather          the cluster's rows (and, when more than 256 k of them, the sorted training sample) through the indices
//   k <= 256: k_hc_assign_direct   64 rows x 64 centroids x 64 coordinates per LDS tile; a thread owns up to 16 (row, centroid)
//                        chains, each the pinned sequential f32 dot in coordinate order, then (nx + nc) - 2 dot clamped at 0 and the
//                        strict-< argmin as a min of (distance bits, cluster); the winning distance feeds the reseed candidates.
//                        The centroid tile is staged per coordinate chunk, so it fits the LDS at every k x dim.
//   k > 256:  KmGemmAssign (k_gemm_shortlist.hip): the GEMM shortlist of k-means
//   update               stable sort of (cluster, row), k_km_bounds, k_km_candidates, k_hc_reseed, k_km_update: no host
//                        synchronisation inside the Lloyd loop.  k_hc_reseed (one wavefront) gives the empty clusters in ascending
//                        order the next candidate under (distance desc, row asc), then next() % rows from the xoshiro state in
//                        device memory (64-bit integer arithmetic), and counts both.
//   partition            the final assignment's stable sort permutes the segment into the subclusters in parent order (k_hc_permute)
//   k_hc_balance_argmin  over the oversized segment: min of (bits of math::l2_distance_sqr in its AVX2 order, position), rows
//                        already moved excluded by their original position (removal keeps the order of the rest); the host
//                        applies the at most 10 moves to the index segments
//   k_hc_centroids       final clusters: per (cluster, coordinate) the f32 sum in member order, then a true division by the count
// The Forgy and sampling shuffles are serial Fisher-Yates and stay on the host.  A cluster of at most host_below rows goes to
// rbq_host::hc_subtree with its whole subtree; the outer RNG carries on, and the result does not depend on where a split ran.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbq.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "km_common.hpp"
#include "../host/rbq_hcluster.hpp"

namespace rbq {

constexpr uint32_t kDaRows = 64, kDaCent = 64, kDaJC = 64, kDaPerThread = 16; // tile of k_hc_assign_direct
constexpr uint32_t kHcDirectMaxK = 256;

// out[i][.] = data[idx[i]][.]
__global__ __launch_bounds__(256) void k_hc_gather(const float* __restrict__ data, const uint32_t* __restrict__ idx, uint64_t m,
                                                   uint32_t dim, float* __restrict__ out) {
    const uint64_t total = m * dim;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = e / dim;
        const uint32_t j = (uint32_t)(e - r * dim);
        out[e] = data[(size_t)idx[r] * dim + j];
    }
}

// out[i] = seg[order[i]]
__global__ __launch_bounds__(256) void k_hc_permute(const uint32_t* __restrict__ seg, const uint32_t* __restrict__ order, uint32_t m,
                                                    uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < m) out[i] = seg[order[i]];
}

// Direct k-means assignment for k <= 256.  Block: 64 rows; lane = row, wave g owns `cpt` centroids of the pass's up to 64.
__global__ __launch_bounds__(256) void k_hc_assign_direct(const float* __restrict__ x, uint32_t m, uint32_t dim,
                                                          const float* __restrict__ nx, const float* __restrict__ cent,
                                                          const float* __restrict__ nc, uint32_t k, uint32_t* __restrict__ best,
                                                          float* __restrict__ bestd) {
    __shared__ float s_x[kDaRows][kDaJC + 1];                 // (+1: lanes read a column, one bank each)
    __shared__ __attribute__((aligned(16))) float s_c[kDaCent][kDaJC];
    __shared__ unsigned long long s_key[4][64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, g = tid >> 6;
    const uint32_t row0 = blockIdx.x * kDaRows, row = row0 + lane;
    const unsigned long long none = ((unsigned long long)__float_as_uint(INFINITY) << 32) | 0xffffffffull;
    unsigned long long key = none;
    const float x2 = row < m ? nx[row] : 0.0f;
    for (uint32_t c0 = 0; c0 < k; c0 += kDaCent) {
        const uint32_t kc = min(kDaCent, k - c0), cpt = (kc + 3u) / 4u, cfirst = g * cpt; // this wave: centroids c0 + cfirst + [0, cpt)
        float acc[kDaPerThread];
#pragma unroll
        for (uint32_t i = 0; i < kDaPerThread; ++i) acc[i] = 0.0f;
        for (uint32_t j0 = 0; j0 < dim; j0 += kDaJC) {
            const uint32_t jn = min(kDaJC, dim - j0);
            __syncthreads(); // the previous tile has been consumed
            for (uint32_t e = tid; e < kDaRows * kDaJC; e += 256u) {
                const uint32_t r = e >> 6, j = e & 63u;
                float v = 0.0f, w = 0.0f;
                if (j < jn) {
                    if (row0 + r < m) v = x[(size_t)(row0 + r) * dim + j0 + j];
                    if (r < kc) w = cent[(size_t)(c0 + r) * dim + j0 + j];
                }
                s_x[r][j] = v;
                s_c[r][j] = w;
            }
            __syncthreads();
            for (uint32_t jj = 0; jj < jn; jj += 16u) {
                if (jj + 16u <= jn) {
                    float xr[16];
#pragma unroll
                    for (uint32_t t = 0; t < 16u; ++t) xr[t] = s_x[lane][jj + t];
#pragma unroll
                    for (uint32_t i = 0; i < kDaPerThread; ++i) {
                        if (i < cpt) { // (wave-uniform)
                            const float4* c4 = reinterpret_cast<const float4*>(&s_c[cfirst + i][jj]);
                            float a = acc[i];
#pragma unroll
                            for (uint32_t q = 0; q < 4u; ++q) {
                                const float4 cv = c4[q];
                                float p;
                                p = xr[4 * q] * cv.x; a = a + p;
                                p = xr[4 * q + 1] * cv.y; a = a + p;
                                p = xr[4 * q + 2] * cv.z; a = a + p;
                                p = xr[4 * q + 3] * cv.w; a = a + p;
                            }
                            acc[i] = a;
                        }
                    }
                } else {
                    for (uint32_t t = jj; t < jn; ++t) {
                        const float xv = s_x[lane][t];
#pragma unroll
                        for (uint32_t i = 0; i < kDaPerThread; ++i)
                            if (i < cpt) { const float p = xv * s_c[cfirst + i][t]; acc[i] = acc[i] + p; }
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < kDaPerThread; ++i) {
            const uint32_t cl = cfirst + i;
            if (i < cpt && cl < kc && row < m) {
                const uint32_t c = c0 + cl;
                float d = (x2 + nc[c]) - 2.0f * acc[i];
                if (d < 0.0f) d = 0.0f;
                if (d < INFINITY) { // (not NaN, below +inf: what a strict < from +inf can pick)
                    const unsigned long long kv = ((unsigned long long)__float_as_uint(d) << 32) | c;
                    key = kv < key ? kv : key;
                }
            }
        }
    }
    s_key[g][lane] = key;
    __syncthreads();
    if (g == 0 && row < m) {
#pragma unroll
        for (uint32_t w = 1; w < 4u; ++w) { const unsigned long long o = s_key[w][lane]; key = o < key ? o : key; }
        best[row] = key == none ? 0u : (uint32_t)key;
        if (bestd) bestd[row] = key == none ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
    }
}

// One wavefront: update_centroids' reseeding.  cands [ncand] keys (distance bits << 32 | ~row; 0 = none) of k_km_candidates;
// rng [6]: the xoshiro256** state, then the counters (empty clusters reseeded, reseeds drawn from the RNG), both advanced.
__global__ __launch_bounds__(64) void k_hc_reseed(const uint32_t* __restrict__ start, const uint32_t* __restrict__ end, uint32_t k,
                                                  const unsigned long long* __restrict__ cands, uint32_t ncand, uint32_t rows,
                                                  uint32_t* __restrict__ src, unsigned long long* __restrict__ rng) {
    const uint32_t lane = threadIdx.x;
    unsigned long long s0 = rng[0], s1 = rng[1], s2 = rng[2], s3 = rng[3], reseeded = 0, draws = 0;
    unsigned long long last = ~0ull; // candidates are taken in descending key order: the next one is the largest below `last`
    bool pool_left = true;
    for (uint32_t c = 0; c < k; ++c) {
        if (end[c] > start[c]) continue;
        ++reseeded;
        unsigned long long pick = 0;
        if (pool_left) {
            for (uint32_t i = lane; i < ncand; i += 64u) {
                const unsigned long long v = cands[i];
                if (v < last && v > pick) pick = v;
            }
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long other = __shfl_xor(pick, o);
                pick = other > pick ? other : pick;
            }
            if (pick == 0) pool_left = false;
        }
        uint32_t row;
        if (pick) {
            last = pick;
            row = 0xffffffffu - (uint32_t)(pick & 0xffffffffull);
        } else { // rbq_host::Rng::next() % rows
            const unsigned long long m5 = s1 * 5ull;
            const unsigned long long r = ((m5 << 7) | (m5 >> 57)) * 9ull, t = s1 << 17;
            s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t; s3 = (s3 << 45) | (s3 >> 19);
            row = (uint32_t)(r % (unsigned long long)rows);
            ++draws;
        }
        if (lane == 0) src[c] = row;
    }
    if (lane == 0) {
        rng[0] = s0; rng[1] = s1; rng[2] = s2; rng[3] = s3;
        rng[4] += reseeded; rng[5] += draws;
    }
}

struct HcExcluded { uint32_t n; uint32_t pos[rbq_host::kHcBalanceRounds]; };

// find_closest_vector_to_centroid over seg[0, len) without the excluded positions: atomicMin of (distance bits << 32 | position)
// into *out (preset to all ones).  Eight lanes per row (cl_canon8).
__global__ __launch_bounds__(256) void k_hc_balance_argmin(const float* __restrict__ data, uint32_t dim, const uint32_t* __restrict__ seg,
                                                           uint32_t len, const float* __restrict__ cu, HcExcluded ex,
                                                           unsigned long long* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    unsigned long long key = ~0ull;
    for (uint64_t base = (uint64_t)wave * 8u; base < len; base += (uint64_t)nwaves * 8u) { // (wave-uniform bound)
        const uint64_t pos = base + (lane >> 3);
        const bool valid = pos < len;
        const float* a = valid ? data + (size_t)seg[valid ? pos : 0] * dim : cu;
        const float d = cl_canon8(a, cu, dim, lane);
        bool take = valid;
        for (uint32_t i = 0; i < ex.n; ++i) take = take && ex.pos[i] != (uint32_t)pos;
        if (take) {
            const unsigned long long kv = ((unsigned long long)__float_as_uint(d) << 32) | (uint32_t)pos;
            key = kv < key ? kv : key;
        }
    }
    key = cl_wave_min(key);
    if (lane == 0 && key != ~0ull) atomicMin(out, key);
}

// compute_centroid: one lane per (cluster, coordinate), the f32 sum over the members in their order, then the division
__global__ __launch_bounds__(64) void k_hc_centroids(const float* __restrict__ data, uint32_t dim, const uint32_t* __restrict__ members,
                                                     const uint32_t* __restrict__ offsets, float* __restrict__ cent) {
    const uint32_t c = blockIdx.x, j = blockIdx.y * 64u + threadIdx.x;
    if (j >= dim) return;
    const uint32_t b = offsets[c], e = offsets[c + 1];
    float s = 0.0f;
    for (uint32_t m = b; m < e; ++m) s = s + data[(size_t)members[m] * dim + j];
    cent[(size_t)c * dim + j] = s / (float)(e - b);
}

namespace {
void hc_shuffle(std::vector<uint32_t>& v, rbq_host::Rng& rng) {
    for (size_t i = v.size(); i-- > 1;) std::swap(v[i], v[rng.next() % (i + 1)]);
}
struct Seg { uint64_t off, len; };
struct Final { bool on_host; uint64_t off, len; std::vector<uint32_t> rows; };
} // namespace

int hcluster_device(const HClusterArgs& a, rbq_host::HcResult& out, std::string& detail) {
    using namespace rbq_host;
    const uint64_t n = a.n, k = a.k;
    const uint32_t dim = a.dim;
    const bool direct = k <= kHcDirectMaxK;
    hipStream_t s = 0;
    KmTemp t;
    uint32_t* flag = nullptr; // finite input only, as for k-means
    bool bad = false;
    KM_TRY(t.alloc(&flag, 1));
    KM_TRY(nonfinite_sync(a.d_data, n * dim, flag, s, &bad));
    if (bad) { detail = "clustering input must be finite"; return RBQ_INVALID_CONFIG; }
    const HcParams prm{a.max_size, k, a.niter, a.balance_weight};
    HcStats st;
    Rng rng(kHcSeed);
    std::vector<Final> fin;
    std::vector<Seg> stack;
    stack.push_back({0, n});

    // ---- the arena: everything a split of the root needs, allocated once (the root is only split when it is over the limit)
    const bool any_device_split = n > a.max_size && n > a.host_below;
    const uint64_t kp = k > UINT64_MAX / kHcPointsPerCentroid ? UINT64_MAX : k * kHcPointsPerCentroid;
    const uint64_t tmax = std::max(std::min(n, kp), k); // most training rows of any split (a split has more than k - 1 rows)
    uint32_t *members = nullptr, *mtmp = nullptr, *d_src = nullptr, *d_start = nullptr, *d_end = nullptr, *asg = nullptr, *fasg = nullptr,
             *keys = nullptr, *iota = nullptr, *vals = nullptr;
    float *xs = nullptr, *xt = nullptr, *full_nx = nullptr, *nx_t = nullptr, *bestd = nullptr, *cent = nullptr;
    unsigned long long *cands = nullptr, *d_rng = nullptr, *d_arg = nullptr;
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
    KmGemmAssign ga;                                                    // k > 256
    CentView dv{(uint32_t)k, dim, 0, nullptr, nullptr, nullptr, nullptr}; // k <= 256: the centroid norms of the direct path
    unsigned kbits = 1;
    while (kbits < 32 && (1ull << kbits) < k) ++kbits; // sort keys < k
    const uint64_t max_cand_chunks = tmax / kHcDecodeBlock + 1;
    KM_TRY(t.alloc(&members, n));
    KM_TRY(launch_iota(members, n, s));
    if (any_device_split) {
        KM_TRY(t.alloc(&mtmp, n));
        KM_TRY(t.alloc(&xs, n * dim));
        if (tmax < n) { KM_TRY(t.alloc(&xt, tmax * dim)); KM_TRY(t.alloc(&nx_t, tmax)); }
        KM_TRY(t.alloc(&full_nx, n));
        KM_TRY(t.alloc(&bestd, tmax));
        KM_TRY(t.alloc(&asg, tmax));
        KM_TRY(t.alloc(&fasg, n));
        KM_TRY(t.alloc(&keys, n));
        KM_TRY(t.alloc(&iota, n));
        KM_TRY(t.alloc(&vals, n));
        KM_TRY(t.alloc(&d_src, std::max(k, tmax)));
        KM_TRY(t.alloc(&d_start, k));
        KM_TRY(t.alloc(&d_end, k));
        KM_TRY(t.alloc(&cent, k * dim));
        KM_TRY(t.alloc(&cands, max_cand_chunks * kCands));
        KM_TRY(t.alloc(&d_rng, 6));
        KM_TRY(t.alloc(&d_arg, 1));
        KM_TRY(hipMemsetAsync(d_rng, 0, 48, s));
        if (direct) { KM_TRY(t.alloc(&dv.nc, k)); KM_TRY(t.alloc(&dv.ncmax_bits, 1)); }
        else KM_TRY(ga.alloc(t, n, k, dim, a.device, s));
        KM_TRY(sort_pairs_u32(nullptr, &sort_bytes, fasg, keys, iota, vals, n, kbits, s));
        KM_TRY(t.alloc((unsigned char**)&sort_tmp, sort_bytes));
        KM_TRY(launch_iota(iota, n, s));
    }
    st.arena_bytes = t.bytes;

    // assignment of rows [0, m) of xa (norms xn) to `cent`
    auto assign = [&](const float* xa, const float* xn, uint64_t m, uint32_t* o, float* bd) -> hipError_t {
        hipError_t e;
        if (!direct) return ga.run(xa, xn, m, cent, o, bd, s);
        if ((e = launch_centroid_norms(cent, dv, s))) return e;
        hipLaunchKernelGGL(k_hc_assign_direct, dim3(grid_of(m, kDaRows)), dim3(256), 0, s, xa, (uint32_t)m, dim, xn, cent, dv.nc, (uint32_t)k, o,
                           bd);
        return hipGetLastError();
    };
    // (cluster, row) pairs of `from` [0, m) sorted stably -> member ranges in d_start / d_end, rows in `vals`
    auto ranges = [&](const uint32_t* from, uint64_t m) -> hipError_t {
        hipError_t e;
        size_t sb = sort_bytes;
        if ((e = sort_pairs_u32(sort_tmp, &sb, from, keys, iota, vals, m, kbits, s))) return e;
        if ((e = hipMemsetAsync(d_start, 0, k * 4, s))) return e;
        if ((e = hipMemsetAsync(d_end, 0, k * 4, s))) return e;
        hipLaunchKernelGGL(k_km_bounds, dim3(grid_of(m, 256)), dim3(256), 0, s, keys, (uint32_t)m, d_start, d_end);
        return hipGetLastError();
    };

    std::vector<uint32_t> h_start(k), h_end(k), idx, seg_rows;
    std::vector<float> h_rows;
    unsigned long long h_rng[6];
    uint64_t dev_reseeded = 0, dev_draws = 0;
    while (!stack.empty()) {
        const Seg sg = stack.back();
        stack.pop_back();
        const uint64_t m = sg.len;
        if (m <= a.max_size) { fin.push_back({false, sg.off, m, {}}); continue; }
        if (m <= a.host_below) {   // the subtree on the host: the same text as rbq_build_hcluster, the same RNG object
            seg_rows.resize(m);
            KM_TRY(hipMemcpy(seg_rows.data(), members + sg.off, m * 4, hipMemcpyDeviceToHost));
            std::vector<std::vector<uint32_t>> sub;
            const uint64_t before = st.splits;
            bool ok;
            if (a.h_data) {
                ok = hc_subtree(a.h_data, dim, seg_rows, prm, rng, sub, st);
            } else {           // rows copied back once, clustered under local indices
                if (!xs) KM_TRY(t.alloc(&xs, n * dim));
                hipLaunchKernelGGL(k_hc_gather, dim3((unsigned)std::min<uint64_t>(4096, grid_of(m * dim, 256))), dim3(256), 0, s, a.d_data,
                                   members + sg.off, m, dim, xs);
                KM_TRY(hipGetLastError());
                h_rows.resize((size_t)m * dim);
                KM_TRY(hipMemcpy(h_rows.data(), xs, m * dim * 4, hipMemcpyDeviceToHost));
                std::vector<uint32_t> local(m);
                for (uint64_t i = 0; i < m; ++i) local[i] = (uint32_t)i;
                ok = hc_subtree(h_rows.data(), dim, std::move(local), prm, rng, sub, st);
                for (auto& c : sub)
                    for (uint32_t& r : c) r = seg_rows[r];
            }
            st.host_splits += st.splits - before;
            if (!ok) { detail = hc_stuck(); return RBQ_INVALID_CONFIG; }
            for (auto& c : sub) fin.push_back({true, 0, c.size(), std::move(c)});
            continue;
        }
        // ---- a split on the device
        const uint64_t seed = rng.next();
        ++st.splits;
        uint32_t* seg = members + sg.off;
        hipLaunchKernelGGL(k_hc_gather, dim3((unsigned)std::min<uint64_t>(4096, grid_of(m * dim, 256))), dim3(256), 0, s, a.d_data, seg, m,
                           dim, xs);
        KM_TRY(hipGetLastError());
        KM_TRY(launch_row_norms(xs, m, dim, full_nx, s));
        const uint64_t target = std::max(std::min(m, kp), k);
        const uint32_t rows = (uint32_t)target;
        const float *x = xs, *nx = full_nx;
        if (target != m) {   // select_training_indices
            Rng sampling_rng(seed);
            idx.resize(m);
            for (uint64_t i = 0; i < m; ++i) idx[i] = (uint32_t)i;
            hc_shuffle(idx, sampling_rng);
            idx.resize(target);
            std::sort(idx.begin(), idx.end());
            KM_TRY(hipMemcpy(d_src, idx.data(), target * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_hc_gather, dim3((unsigned)std::min<uint64_t>(4096, grid_of(target * dim, 256))), dim3(256), 0, s, xs, d_src,
                               target, dim, xt);
            KM_TRY(hipGetLastError());
            KM_TRY(launch_row_norms(xt, rows, dim, nx_t, s));
            x = xt;
            nx = nx_t;
        }
        Rng redo_rng(seed);
        {   // Forgy: centroid c = training row idx[c] (k_km_update with every member range empty)
            idx.resize(rows);
            for (uint32_t i = 0; i < rows; ++i) idx[i] = i;
            hc_shuffle(idx, redo_rng);
            KM_TRY(hipMemcpy(d_src, idx.data(), k * 4, hipMemcpyHostToDevice));
            KM_TRY(hipMemsetAsync(d_start, 0, k * 4, s));
            KM_TRY(hipMemsetAsync(d_end, 0, k * 4, s));
            hipLaunchKernelGGL(k_km_update, dim3((unsigned)k, grid_of(dim, 64)), dim3(64), 0, s, x, dim, (const uint32_t*)nullptr, d_start,
                               d_end, d_src, cent);
            KM_TRY(hipGetLastError());
            KM_TRY(hipMemcpy(d_rng, redo_rng.s, 32, hipMemcpyHostToDevice)); // the reseed draws carry on from here
        }
        const uint32_t dbs = (uint32_t)std::min<uint64_t>(kHcDecodeBlock, rows);
        const uint32_t nchunks = (rows + dbs - 1) / dbs;
        for (uint64_t it = 0; it < a.niter; ++it) {   // (no host synchronisation in here)
            KM_TRY(assign(x, nx, rows, asg, bestd));
            KM_TRY(ranges(asg, rows));
            hipLaunchKernelGGL(k_km_candidates, dim3(nchunks), dim3(64), 0, s, bestd, rows, dbs, cands);
            KM_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_hc_reseed, dim3(1), dim3(64), 0, s, d_start, d_end, (uint32_t)k, cands, nchunks * kCands, rows, d_src, d_rng);
            KM_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_km_update, dim3((unsigned)k, grid_of(dim, 64)), dim3(64), 0, s, x, dim, vals, d_start, d_end, d_src, cent);
            KM_TRY(hipGetLastError());
        }
        // the final assignment of every row; its stable sort is the partition into subclusters in parent order
        KM_TRY(assign(xs, full_nx, m, fasg, nullptr));
        KM_TRY(ranges(fasg, m));
        hipLaunchKernelGGL(k_hc_permute, dim3(grid_of(m, 256)), dim3(256), 0, s, seg, vals, (uint32_t)m, mtmp);
        KM_TRY(hipGetLastError());
        KM_TRY(hipMemcpyAsync(seg, mtmp, m * 4, hipMemcpyDeviceToDevice, s));
        KM_TRY(hipMemcpyAsync(h_start.data(), d_start, k * 4, hipMemcpyDeviceToHost, s));
        KM_TRY(hipMemcpyAsync(h_end.data(), d_end, k * 4, hipMemcpyDeviceToHost, s));
        KM_TRY(hipMemcpyAsync(h_rng, d_rng, 48, hipMemcpyDeviceToHost, s)); // (the counters run over the whole call)
        KM_TRY(hipStreamSynchronize(s)); // once per split
        dev_reseeded = h_rng[4];
        dev_draws = h_rng[5];
        // ---- balance_clusters: the argmin on the device, the moves on the host
        std::vector<uint64_t> size(k);
        for (uint64_t c = 0; c < k; ++c) size[c] = h_end[c] - h_start[c];
        std::vector<std::vector<uint32_t>> removed(k); // original positions (within the subcluster) taken out of it
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> gain(k); // rows pushed to it: (donor, original position there)
        uint64_t moves = 0, b_target = 0, b_max = 0;
        if (hc_limits(m, k, a.balance_weight, b_target, b_max)) {
            for (uint64_t round = 0; round < kHcBalanceRounds; ++round) {
                uint64_t over, under;
                if (!hc_pick(k, b_target, b_max, [&](uint64_t c) { return size[c]; }, over, under)) break;
                HcExcluded ex{};
                ex.n = (uint32_t)removed[over].size();
                for (uint32_t i = 0; i < ex.n; ++i) ex.pos[i] = removed[over][i];
                const uint32_t len = h_end[over] - h_start[over];
                KM_TRY(hipMemsetAsync(d_arg, 0xff, 8, s));
                hipLaunchKernelGGL(k_hc_balance_argmin, dim3(std::min<unsigned>(1024, grid_of(len, 32))), dim3(256), 0, s, a.d_data, dim,
                                   seg + h_start[over], len, cent + under * dim, ex, d_arg);
                KM_TRY(hipGetLastError());
                unsigned long long got = 0;
                KM_TRY(hipMemcpy(&got, d_arg, 8, hipMemcpyDeviceToHost));
                if (got == ~0ull) break; // (an oversized subcluster is never empty)
                const uint32_t pos = (uint32_t)(got & 0xffffffffull);
                removed[over].push_back(pos);
                gain[under].push_back({(uint32_t)over, pos});
                --size[over];
                ++size[under];
                ++moves;
            }
        }
        if (moves) {   // rewrite the segment: every subcluster without its removed rows, then the rows pushed to its end
            seg_rows.resize(m);
            KM_TRY(hipMemcpy(seg_rows.data(), seg, m * 4, hipMemcpyDeviceToHost));
            std::vector<uint32_t> neu;
            neu.reserve(m);
            for (uint64_t c = 0; c < k; ++c) {
                for (uint32_t p = 0; p < h_end[c] - h_start[c]; ++p)
                    if (std::find(removed[c].begin(), removed[c].end(), p) == removed[c].end()) neu.push_back(seg_rows[h_start[c] + p]);
                for (const auto& g : gain[c]) neu.push_back(seg_rows[h_start[g.first] + g.second]);
            }
            KM_TRY(hipMemcpy(seg, neu.data(), m * 4, hipMemcpyHostToDevice));
            st.balance_moves += moves;
        }
        uint64_t nonempty = 0, off = sg.off;
        for (uint64_t c = 0; c < k; ++c) {
            if (!size[c]) continue;
            ++nonempty;
            stack.push_back({off, size[c]});
            off += size[c];
        }
        if (nonempty < 2) { detail = hc_stuck(); return RBQ_INVALID_CONFIG; }
    }
    st.reseeded += dev_reseeded; // (host subtrees counted into st directly)
    st.draws += dev_draws;
    // ---- the final clusters in pop order, their centroids on the device
    const uint64_t ncl = fin.size();
    std::vector<uint32_t> h_members(n);
    KM_TRY(hipMemcpy(h_members.data(), members, n * 4, hipMemcpyDeviceToHost));
    out.dim = dim;
    out.offsets.assign(1, 0);
    out.members.clear();
    out.members.reserve(n);
    for (const Final& f : fin) {
        if (f.on_host) out.members.insert(out.members.end(), f.rows.begin(), f.rows.end());
        else out.members.insert(out.members.end(), h_members.begin() + (ptrdiff_t)f.off, h_members.begin() + (ptrdiff_t)(f.off + f.len));
        out.offsets.push_back(out.members.size());
    }
    std::vector<uint32_t> off32(ncl + 1);
    for (uint64_t c = 0; c <= ncl; ++c) off32[c] = (uint32_t)out.offsets[c];
    uint32_t* d_off = nullptr;
    float* d_cent = nullptr;
    KM_TRY(t.alloc(&d_off, ncl + 1));
    KM_TRY(t.alloc(&d_cent, ncl * dim));
    KM_TRY(hipMemcpy(d_off, off32.data(), (ncl + 1) * 4, hipMemcpyHostToDevice));
    KM_TRY(hipMemcpy(members, out.members.data(), n * 4, hipMemcpyHostToDevice));
    for (uint64_t c0 = 0; c0 < ncl; c0 += 65535u * 64u) { // (grid.x is the cluster)
        const unsigned nb = (unsigned)std::min<uint64_t>(65535u * 64u, ncl - c0);
        hipLaunchKernelGGL(k_hc_centroids, dim3(nb, grid_of(dim, 64)), dim3(64), 0, s, a.d_data, dim, members, d_off + c0, d_cent + c0 * dim);
        KM_TRY(hipGetLastError());
    }
    out.centroids.resize((size_t)ncl * dim);
    KM_TRY(hipMemcpy(out.centroids.data(), d_cent, ncl * dim * 4, hipMemcpyDeviceToHost));
    st.arena_bytes = std::max<uint64_t>(st.arena_bytes, t.bytes);
    out.set_stats(st);
    return RBQ_OK;
}

} // namespace rbq
