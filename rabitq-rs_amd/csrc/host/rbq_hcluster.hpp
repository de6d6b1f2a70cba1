// rbq_hcluster.hpp — the pinned host arithmetic of the Faiss-style k-means (run_kmeans_with_config, reference src/kmeans.rs) and
// of MSTG's hierarchical balanced clustering (HierarchicalClustering::cluster, reference src/mstg/clustering.rs).  Header-only:
// the CPU builder (rbq_build.cpp: rbq_build_kmeans_faiss, rbq_build_hcluster) and the device library (api_mstg.hip, which hands
// subtrees of small clusters to the host) compile the same text, so both sides of rbq_mstg_cluster_device agree bit for bit.
// The pins of the k-means are stated at rbq_build_kmeans_faiss (rbq_build.cpp); the clustering adds:
//   rng        Rng(42); split number i in pop order takes draw number i of next() as its k-means seed
//   k-means    niter = max_iterations, nredo 1, not spherical, 256 points per centroid, decode block 32768
//   balance    target = total / k; max_allowed = (usize)(target as f32 * (1.0f + balance_weight)) with Rust's saturating cast; at
//              most 10 rounds: first subcluster over max_allowed, first under target, the row of the former with the strictly
//              smallest math::l2_distance_sqr (AVX2 order) to the latter's k-means centroid (first row wins a tie) is removed
//              and pushed to the end of the latter
//   centroid   per coordinate an f32 sum over the rows in the cluster's order, then a true division by (float)n
#ifndef RBQ_HCLUSTER_HPP
#define RBQ_HCLUSTER_HPP
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "rbq_rng.h"

namespace rbq_host {

inline void km_shuffle(std::vector<uint64_t>& v, Rng& rng) {
    for (size_t i = v.size(); i-- > 1;) std::swap(v[i], v[rng.next() % (i + 1)]);
}

inline float km_norm(const float* x, uint32_t dim) {
    float s = 0.0f;
    for (uint32_t j = 0; j < dim; ++j) { float p = x[j] * x[j]; s = s + p; }
    return s;
}

inline uint64_t km_cand_key(float dist, uint64_t row) {
    uint32_t b;
    std::memcpy(&b, &dist, 4);
    return ((uint64_t)b << 32) | (0xffffffffull - row);
}

// assignment of rows [0, rows) of x (norms nx) to the centroids (column copy ccol [dim][k], norms nc): best cluster + its distance.
// Independent sequential chains over coordinates, 64 clusters at a time (vectorised across clusters, never within a chain).
inline void km_assign(const float* x, const float* nx, uint64_t rows, uint32_t dim, uint64_t k, const float* ccol, const float* nc,
                      uint32_t* best, float* bestd) {
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < (int64_t)rows; ++i) {
        const float* xr = x + (size_t)i * dim;
        float bd = INFINITY;
        uint32_t bc = 0;
        for (uint64_t c0 = 0; c0 < k; c0 += 64) {
            const uint64_t nb = std::min<uint64_t>(64, k - c0);
            float acc[64];
            for (uint64_t c = 0; c < 64; ++c) acc[c] = 0.0f;
            for (uint32_t j = 0; j < dim; ++j) {
                const float xv = xr[j];
                const float* cc = ccol + (size_t)j * k + c0;
                if (nb == 64) {
                    for (int c = 0; c < 64; ++c) { float p = xv * cc[c]; acc[c] = acc[c] + p; }
                } else {
                    for (uint64_t c = 0; c < nb; ++c) { float p = xv * cc[c]; acc[c] = acc[c] + p; }
                }
            }
            for (uint64_t c = 0; c < nb; ++c) {
                float d = (nx[i] + nc[c0 + c]) - 2.0f * acc[c];
                if (d < 0.0f) d = 0.0f;
                if (d < bd) { bd = d; bc = (uint32_t)(c0 + c); }
            }
        }
        best[i] = bc;
        if (bestd) bestd[i] = bd;
    }
}

inline void km_views(const float* cent, uint64_t k, uint32_t dim, std::vector<float>& ccol, std::vector<float>& nc) {
    ccol.assign((size_t)k * dim, 0.0f);
    nc.assign(k, 0.0f);
    for (uint64_t c = 0; c < k; ++c) {
        for (uint32_t j = 0; j < dim; ++j) ccol[(size_t)j * k + c] = cent[(size_t)c * dim + j];
        nc[c] = km_norm(cent + (size_t)c * dim, dim);
    }
}

// run_kmeans_with_config on validated, finite input (rbq_build_kmeans_faiss checks; see there for the pins).
// objective may be null (it is then not computed); stats [2] (nullable): empty clusters reseeded, reseeds drawn from the RNG.
inline void kmeans_faiss_core(const float* data, uint64_t n, uint32_t dim, uint64_t k, uint64_t niter, uint64_t nredo, uint64_t seed,
                              int spherical, uint64_t max_points_per_centroid, uint64_t decode_block_size, float* centroids,
                              uint32_t* assignments, double* objective, uint64_t* stats) {
    uint64_t st_reseed = 0, st_draws = 0;
    // select_training_indices
    Rng sampling_rng(seed);
    const uint64_t kp = max_points_per_centroid && k > UINT64_MAX / max_points_per_centroid ? UINT64_MAX : k * max_points_per_centroid;
    const uint64_t target = std::max(std::min(n, kp), k);
    std::vector<float> sample;
    const float* x = data;
    uint64_t rows = n;
    if (target != n) {
        std::vector<uint64_t> idx(n);
        for (uint64_t i = 0; i < n; ++i) idx[i] = i;
        km_shuffle(idx, sampling_rng);
        idx.resize(target);
        std::sort(idx.begin(), idx.end());
        sample.resize((size_t)target * dim);
        for (uint64_t i = 0; i < target; ++i) std::memcpy(&sample[(size_t)i * dim], data + idx[i] * dim, sizeof(float) * dim);
        x = sample.data();
        rows = target;
    }
    std::vector<float> nx(rows), full_nx(n);
    for (uint64_t i = 0; i < rows; ++i) nx[i] = km_norm(x + (size_t)i * dim, dim);
    for (uint64_t i = 0; i < n; ++i) full_nx[i] = km_norm(data + (size_t)i * dim, dim);
    std::vector<float> cent((size_t)k * dim), ccol, nc, bestd(rows), sums;
    std::vector<uint32_t> asg(rows), fin(n);
    std::vector<uint64_t> counts;
    double best_obj = 0.0;
    for (uint64_t r = 0; r < nredo; ++r) {
        Rng redo_rng(seed + r * 0x9e3779b97f4a7c15ull);
        {   // Forgy
            std::vector<uint64_t> idx(rows);
            for (uint64_t i = 0; i < rows; ++i) idx[i] = i;
            km_shuffle(idx, redo_rng);
            for (uint64_t c = 0; c < k; ++c) std::memcpy(&cent[(size_t)c * dim], x + idx[c] * dim, sizeof(float) * dim);
        }
        for (uint64_t it = 0; it < niter; ++it) {
            km_views(cent.data(), k, dim, ccol, nc);
            km_assign(x, nx.data(), rows, dim, k, ccol.data(), nc.data(), asg.data(), bestd.data());
            counts.assign(k, 0);
            for (uint64_t i = 0; i < rows; ++i) counts[asg[i]]++;
            sums.assign((size_t)k * dim, 0.0f);
#pragma omp parallel
            {   // coordinate ranges over threads: every (cluster, coordinate) sum stays one ascending-row chain
#ifdef _OPENMP
                const uint32_t nt = (uint32_t)omp_get_num_threads(), t = (uint32_t)omp_get_thread_num();
#else
                const uint32_t nt = 1, t = 0;
#endif
                const uint32_t j0 = (uint32_t)((uint64_t)dim * t / nt), j1 = (uint32_t)((uint64_t)dim * (t + 1) / nt);
                for (uint64_t i = 0; i < rows; ++i) {
                    float* s = &sums[(size_t)asg[i] * dim];
                    const float* xr = x + (size_t)i * dim;
                    for (uint32_t j = j0; j < j1; ++j) s[j] = s[j] + xr[j];
                }
            }
            // reseed candidates: per chunk the 8 first under (distance desc, row asc)
            std::vector<uint64_t> pool;
            for (uint64_t s0 = 0; s0 < rows; s0 += decode_block_size) {
                const uint64_t e = std::min(rows, s0 + decode_block_size);
                std::vector<uint64_t> keys;
                keys.reserve(e - s0);
                for (uint64_t i = s0; i < e; ++i) keys.push_back(km_cand_key(bestd[i], i));
                const size_t take = std::min<size_t>(8, keys.size());
                std::partial_sort(keys.begin(), keys.begin() + take, keys.end(), std::greater<uint64_t>());
                pool.insert(pool.end(), keys.begin(), keys.begin() + take);
            }
            std::sort(pool.begin(), pool.end(), std::greater<uint64_t>());
            size_t next = 0;
            for (uint64_t c = 0; c < k; ++c) {
                float* cc = &cent[(size_t)c * dim];
                if (counts[c] > 0) {
                    const float inv = 1.0f / (float)counts[c];
                    for (uint32_t j = 0; j < dim; ++j) cc[j] = sums[(size_t)c * dim + j] * inv;
                } else {
                    uint64_t src;
                    if (next < pool.size()) src = 0xffffffffull - (pool[next++] & 0xffffffffull);
                    else { src = redo_rng.next() % rows; ++st_draws; }
                    ++st_reseed;
                    std::memcpy(cc, x + src * dim, sizeof(float) * dim);
                }
            }
            if (spherical) {
                for (uint64_t c = 0; c < k; ++c) {
                    float* cc = &cent[(size_t)c * dim];
                    const float nrm = km_norm(cc, dim);
                    if (nrm > 0.0f) {
                        const float inv = 1.0f / std::sqrt(nrm);
                        for (uint32_t j = 0; j < dim; ++j) cc[j] = cc[j] * inv;
                    }
                }
            }
        }
        // assignment of the full dataset + objective
        km_views(cent.data(), k, dim, ccol, nc);
        km_assign(data, full_nx.data(), n, dim, k, ccol.data(), nc.data(), fin.data(), nullptr);
        double obj = 0.0;
        if (objective) {
            std::vector<double> rd(n);
#pragma omp parallel for schedule(static)
            for (int64_t i = 0; i < (int64_t)n; ++i) {
                const float* xr = data + (size_t)i * dim;
                const float* cc = &cent[(size_t)fin[i] * dim];
                double s = 0.0;
                for (uint32_t j = 0; j < dim; ++j) { double dl = (double)(xr[j] - cc[j]); s = s + dl * dl; }
                rd[i] = s;
            }
            for (uint64_t i = 0; i < n; ++i) obj = obj + rd[i];
        }
        if (r == 0 || obj < best_obj) {
            best_obj = obj;
            std::memcpy(centroids, cent.data(), sizeof(float) * (size_t)k * dim);
            std::memcpy(assignments, fin.data(), sizeof(uint32_t) * n);
        }
    }
    if (objective) *objective = best_obj;
    if (stats) { stats[0] = st_reseed; stats[1] = st_draws; }
}

// math::l2_distance_sqr, AVX2 lane order (src/math.rs:216-245)
inline float l2_sqr8(const float* a, const float* b, size_t len) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t chunks = len / 8, i = 0;
    for (; i < chunks * 8; i += 8)
        for (int l = 0; l < 8; ++l) { float d = a[i + l] - b[i + l]; float p = d * d; acc[l] = acc[l] + p; }
    float sum = 0.0f;
    if (chunks) { sum = -0.0f; for (int l = 0; l < 8; ++l) sum = sum + acc[l]; }
    for (; i < len; ++i) { float d = a[i] - b[i]; float p = d * d; sum = sum + p; }
    return sum;
}

// ---------------------------------------------------------------- hierarchical balanced clustering
constexpr uint64_t kHcSeed = 42, kHcPointsPerCentroid = 256, kHcDecodeBlock = 32768, kHcBalanceRounds = 10;

struct HcParams {
    uint64_t max_size, k, niter;
    float balance_weight;
};
struct HcStats {
    uint64_t splits = 0, balance_moves = 0, reseeded = 0, draws = 0, host_splits = 0, arena_bytes = 0;
};

// balance_clusters' limits; false when balancing is off (balance_weight NaN or <= 0)
inline bool hc_limits(uint64_t total, uint64_t k, float w, uint64_t& target, uint64_t& max_allowed) {
    if (!(w > 0.0f)) return false;
    target = total / k;
    const float one_w = 1.0f + w;
    const float v = (float)target * one_w;
    if (v != v || v <= 0.0f) max_allowed = 0;                          // `as usize`: NaN and negatives give 0
    else if (!(v < 18446744073709551616.0f)) max_allowed = UINT64_MAX; // saturates
    else max_allowed = (uint64_t)v;
    return true;
}
// the (over, under) pair of one balancing round, or false when the subclusters are balanced
template <class SizeOf> inline bool hc_pick(uint64_t k, uint64_t target, uint64_t max_allowed, SizeOf size, uint64_t& over, uint64_t& under) {
    over = under = k;
    for (uint64_t c = 0; c < k; ++c) if (size(c) > max_allowed) { over = c; break; }
    for (uint64_t c = 0; c < k; ++c) if (size(c) < target) { under = c; break; }
    return over < k && under < k;
}

inline const char* hc_stuck() { return "a split left a single non-empty subcluster: the clustering would never end"; }

// split_cluster: rows (indices into data, the cluster's order) -> the non-empty subclusters in ascending id.  false: stuck.
inline bool hc_split(const float* data, uint32_t dim, const std::vector<uint32_t>& rows, const HcParams& p, uint64_t seed,
                     std::vector<std::vector<uint32_t>>& sub, HcStats& st) {
    const uint64_t m = rows.size(), k = p.k;
    std::vector<float> buf((size_t)m * dim), cent((size_t)k * dim);
    for (uint64_t i = 0; i < m; ++i) std::memcpy(&buf[(size_t)i * dim], data + (size_t)rows[i] * dim, sizeof(float) * dim);
    std::vector<uint32_t> asg(m);
    uint64_t ks[2] = {0, 0};
    kmeans_faiss_core(buf.data(), m, dim, k, p.niter, 1, seed, 0, kHcPointsPerCentroid, kHcDecodeBlock, cent.data(), asg.data(), nullptr, ks);
    st.reseeded += ks[0];
    st.draws += ks[1];
    ++st.splits;
    std::vector<std::vector<uint32_t>> cl(k);
    for (uint64_t i = 0; i < m; ++i) cl[asg[i]].push_back(rows[i]);
    uint64_t target = 0, max_allowed = 0;
    if (hc_limits(m, k, p.balance_weight, target, max_allowed)) {
        for (uint64_t round = 0; round < kHcBalanceRounds; ++round) {
            uint64_t over, under;
            if (!hc_pick(k, target, max_allowed, [&](uint64_t c) { return (uint64_t)cl[c].size(); }, over, under)) break;
            std::vector<uint32_t>& from = cl[over];
            const float* cu = &cent[(size_t)under * dim];
            size_t best = 0;
            float bd = l2_sqr8(data + (size_t)from[0] * dim, cu, dim);
            for (size_t i = 1; i < from.size(); ++i) {
                const float d = l2_sqr8(data + (size_t)from[i] * dim, cu, dim);
                if (d < bd) { bd = d; best = i; }
            }
            const uint32_t row = from[best];
            from.erase(from.begin() + (ptrdiff_t)best);
            cl[under].push_back(row);
            ++st.balance_moves;
        }
    }
    sub.clear();
    for (uint64_t c = 0; c < k; ++c)
        if (!cl[c].empty()) sub.push_back(std::move(cl[c]));
    return sub.size() > 1;
}

// the stack walk from one cluster: final clusters are appended to `fin` in pop order.  false: stuck.
inline bool hc_subtree(const float* data, uint32_t dim, std::vector<uint32_t> root, const HcParams& p, Rng& rng,
                       std::vector<std::vector<uint32_t>>& fin, HcStats& st) {
    std::vector<std::vector<uint32_t>> stack, sub;
    stack.push_back(std::move(root));
    while (!stack.empty()) {
        std::vector<uint32_t> c = std::move(stack.back());
        stack.pop_back();
        if (c.size() <= p.max_size) { fin.push_back(std::move(c)); continue; }
        if (!hc_split(data, dim, c, p, rng.next(), sub, st)) return false;
        for (auto& s : sub) stack.push_back(std::move(s));
    }
    return true;
}

// compute_centroid of rows[0, n): sequential f32 sums, then the division
inline void hc_centroid(const float* data, uint32_t dim, const uint32_t* rows, uint64_t n, float* out) {
    for (uint32_t j = 0; j < dim; ++j) out[j] = 0.0f;
    for (uint64_t i = 0; i < n; ++i) {
        const float* x = data + (size_t)rows[i] * dim;
        for (uint32_t j = 0; j < dim; ++j) out[j] = out[j] + x[j];
    }
    const float fn = (float)n;
    for (uint32_t j = 0; j < dim; ++j) out[j] = out[j] / fn;
}

// what both entry points refuse before any work; null = fine
inline const char* hc_check(const void* data, uint64_t n, uint32_t dim, uint64_t max_size, uint64_t k, uint64_t niter) {
    if (!data) return "null buffer";
    if (n == 0) return "no vectors";
    if (dim == 0) return "dimension must be positive";
    if (n >= 0xffffffffull) return "too many vectors for 32-bit row indices";
    if (niter == 0) return "max_iterations must be positive";
    if (k < 2) return "branching_factor must be at least 2";
    if (max_size == UINT64_MAX ? false : k > max_size + 1) return "branching_factor above max_posting_size + 1: a cluster one row over the limit could not be split";
    return nullptr;
}

// the result both entry points hand out (opaque to C callers)
struct HcResult {
    uint32_t dim = 0;
    std::vector<float> centroids;   // [n_clusters][dim]
    std::vector<uint64_t> offsets;  // [n_clusters + 1]
    std::vector<uint32_t> members;  // [n]
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0}; // splits, balance moves, reseeded, draws, host splits, largest arena (bytes)
    void set_stats(const HcStats& s) {
        stats[0] = s.splits; stats[1] = s.balance_moves; stats[2] = s.reseeded; stats[3] = s.draws; stats[4] = s.host_splits;
        stats[5] = s.arena_bytes;
    }
    void set_members(const std::vector<std::vector<uint32_t>>& fin) {
        offsets.assign(1, 0);
        members.clear();
        for (const auto& c : fin) { members.insert(members.end(), c.begin(), c.end()); offsets.push_back(members.size()); }
    }
};

} // namespace rbq_host
#endif
