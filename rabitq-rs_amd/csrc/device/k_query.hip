// k_query.hip — translation unit of the per-batch query stages in front of the scan: k_prep / k_prep_wave
// (rotate + constants + LUT), the centroid-ranking GEMMs, probe selection and the MSTG probe list.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "launch.hpp"
#include "query_kernels.hpp"
#include "rank_mfma.hpp"
#include "select_given.hpp"
#include "select_mfma.hpp"
#include "latency.hpp"

namespace rbq {

namespace {
uint32_t next_pow2(uint32_t x) { uint32_t p = 1; while (p < x) p <<= 1; return p; }
} // namespace

namespace {
// the preparation kernels are templates on the element of the query rows: every instantiation has its own kernel address, hence its
// own LDS-limit cache and its own identity under a stage probe
template <typename QT>
hipError_t launch_prep_of(const PrepParams& p, int device, hipStream_t s) {
    const QT* queries = static_cast<const QT*>(p.queries);
    if (p.rotator == 0 /* matrix: O(D^2) per query */ || p.wg_prep) {
        static LdsAttrCache attr;
        const size_t lds = (size_t)p.D * 4 * 2;
        if (probe_stage(0, reinterpret_cast<const void*>(&k_prep<QT>), dim3(p.nq), kThreads, lds)) return hipSuccess;
        hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_prep<QT>), lds, device);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_prep<QT>, dim3(p.nq), dim3(kThreads), lds, s, queries, p.dim, p.D, p.Dc, p.rotator, p.rot_blob, p.trunc,
                           p.fac, p.ex_bits, p.rot, p.lut, p.consts, p.rot_hl, p.rank_resid);
    } else { // FHT-Kac / identity: one wave per query
        static LdsAttrCache attr;
        const uint32_t qpw = kThreads / 64;
        const size_t lds = (size_t)p.D * 4 * 2 * qpw + p.D / 2;
        if (probe_stage(0, reinterpret_cast<const void*>(&k_prep_wave<QT>), dim3((p.nq + qpw - 1) / qpw), kThreads, lds)) return hipSuccess;
        hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_prep_wave<QT>), lds, device); // 66.5 KB at D = 2048
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_prep_wave<QT>, dim3((p.nq + qpw - 1) / qpw), dim3(kThreads), lds, s, queries, p.nq, p.dim, p.D, p.Dc,
                           p.rotator, p.rot_blob, p.trunc, p.fac, p.ex_bits, p.rot, p.lut, p.consts, p.rot_hl, p.rank_resid);
    }
    return hipGetLastError();
}
template <typename QT>
hipError_t launch_lat_front_of(const LatFrontParams& P, int device, hipStream_t s) {
    static LdsAttrCache attr;
    const dim3 grid(lat_front_grid(P.scorers, P.prep.nq));
    const size_t lds = (size_t)P.prep.D * 4 * 2 + P.prep.D / 2;
    if (probe_stage(0, reinterpret_cast<const void*>(&k_lat_front<QT>), grid, kThreads, lds)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_lat_front<QT>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lat_front<QT>, grid, dim3(kThreads), lds, s, P);
    return hipGetLastError();
}
} // namespace

hipError_t launch_prep(const PrepParams& p, int device, hipStream_t s) {
    if (p.query_dtype == kRawF16) return launch_prep_of<RawF16>(p, device, s);
    if (p.query_dtype == kRawBf16) return launch_prep_of<RawBf16>(p, device, s);
    if (p.query_dtype != kRawF32) return hipErrorInvalidValue;
    return launch_prep_of<float>(p, device, s);
}

// latency-first front of a small call (latency.hpp): rotation + constants + LUT + the exact canonical score of every list, one launch
hipError_t launch_lat_front(const PrepParams& p, const RankParams& r, int device, hipStream_t s) {
    LatFrontParams P;
    P.prep = p; P.cent = r.cent; P.nlist = r.nlist; P.metric = r.metric; P.scores = r.scores;
    P.scorers = (r.scores && !r.ksplit) ? (r.nlist + kLatLists - 1) / kLatLists : 0u;
    P.zero_scores = r.ksplit > 1 ? r.scores : nullptr; // (split-K ranking GEMM behind this preparation: its parts are added to a zeroed row)
    if (p.query_dtype == kRawF16) return launch_lat_front_of<RawF16>(P, device, s);
    if (p.query_dtype == kRawBf16) return launch_lat_front_of<RawBf16>(P, device, s);
    if (p.query_dtype != kRawF32) return hipErrorInvalidValue;
    return launch_lat_front_of<float>(P, device, s);
}

hipError_t launch_rank_exact(const RankParams& p, hipStream_t s) {
    dim3 grid((p.nlist + 31) / 32, (p.nq + 31) / 32);
    if (probe_stage(1, p.metric == 0 ? reinterpret_cast<const void*>(&k_rank_scores<0>) : reinterpret_cast<const void*>(&k_rank_scores<1>), grid, kThreads, 0, kRankOpsF32)) return hipSuccess;
    if (p.metric == 0) hipLaunchKernelGGL(k_rank_scores<0>, grid, dim3(kThreads), 0, s, p.rot, p.cent, p.nq, p.nlist, p.D, p.scores);
    else hipLaunchKernelGGL(k_rank_scores<1>, grid, dim3(kThreads), 0, s, p.rot, p.cent, p.nq, p.nlist, p.D, p.scores);
    return hipGetLastError();
}

namespace {
// shape of a ranking GEMM: metric M; workgroups of WM x WN waves, each wave TM x TN MFMA blocks of 32 x 32
template <int M, int TM_, int TN_, int WM_, int WN_>
struct RankShape { static constexpr int metric = M, TM = TM_, TN = TN_, WM = WM_, WN = WN_; };
// THE metric and tile table of the three GEMMs, f(shape) with the call's shape as a type.  wide (very large problems, cfg5: 16 384 x
// 65 536): 128 x 256 tiles, each wave a 64 x 64 sub-tile — 8 LDS fragment reads per 12 MFMAs instead of 6 per 6, one workgroup (123 KB of
// LDS) per compute unit; big: 128 x 128 tiles, 8 waves (each 64 x 32) — the tile traffic of the 4-wave form with twice the waves to hide
// the staging behind the MFMAs; else 64 x 64 tiles, 4 waves.  (k_rank_mfma: square tiles of 64 TM on four waves, no wide form.)
template <class F>
hipError_t with_rank_shape(int metric, bool wide, bool big, F&& f) {
    if (metric == 0) return wide ? f(RankShape<0, 2, 2, 2, 4>{}) : big ? f(RankShape<0, 2, 1, 2, 4>{}) : f(RankShape<0, 1, 1, 2, 2>{});
    return wide ? f(RankShape<1, 2, 2, 2, 4>{}) : big ? f(RankShape<1, 2, 1, 2, 4>{}) : f(RankShape<1, 1, 1, 2, 2>{});
}
template <class S>
hipError_t launch_rank_split(const RankParams& p, dim3 grid, int device, hipStream_t s) {
    constexpr auto kernel = &k_rank_bf16_db<S::metric, S::TM, S::TN, S::WM, S::WN>;
    static LdsAttrCache attr;
    const size_t lds = (size_t)(2 * 32 * S::TM * S::WM + 2 * 32 * S::TN * S::WN) * 80 * 2; // two slabs of 32, rows of 80 B
    if (probe_stage(1, reinterpret_cast<const void*>(kernel), grid, 64 * S::WM * S::WN, lds, kRankOpsBf16x3)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(kernel), lds, device);
    if (e != hipSuccess) return e;
    // operands: planar (two planes, rows of 2 D bytes, slabs of 64) or interleaved (one image at *_hi: the lo plane 64 bytes behind the hi
    // plane, rows of 4 D bytes, slabs of 128)
    const unsigned char* ah = reinterpret_cast<const unsigned char*>(p.rot_hi);
    const unsigned char* al = p.rot_hl ? ah + 64 : reinterpret_cast<const unsigned char*>(p.rot_lo);
    const unsigned char* bh = reinterpret_cast<const unsigned char*>(p.cent_hi);
    const unsigned char* bl = p.cent_hl ? bh + 64 : reinterpret_cast<const unsigned char*>(p.cent_lo);
    hipLaunchKernelGGL(kernel, grid, dim3(64 * S::WM * S::WN), lds, s, ah, al, p.D * (p.rot_hl ? 4u : 2u), p.rot_hl ? 128u : 64u, bh, bl,
                       p.D * (p.cent_hl ? 4u : 2u), p.cent_hl ? 128u : 64u, p.consts, p.cnorm2, p.nq, p.nlist, p.D, p.scores);
    return hipGetLastError();
}
// the one-product f16 form of the same tiles (k_rank_f16_db): two slabs of 64, rows of 144 B
template <class S>
hipError_t launch_rank_f16(const RankParams& p, dim3 grid, int device, hipStream_t s) {
    constexpr auto kernel = &k_rank_f16_db<S::metric, S::TM, S::TN, S::WM, S::WN>;
    static LdsAttrCache attr;
    const size_t lds = (size_t)(32 * S::TM * S::WM + 32 * S::TN * S::WN) * 144 * 2;
    if (probe_stage(1, reinterpret_cast<const void*>(kernel), grid, 64 * S::WM * S::WN, lds, kRankOpsF16)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(kernel), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(64 * S::WM * S::WN), lds, s, reinterpret_cast<const unsigned char*>(p.rot_hi),
                       reinterpret_cast<const unsigned char*>(p.cent_hi), p.consts, p.cnorm2, p.nq, p.nlist, p.D, p.scores);
    return hipGetLastError();
}
template <class S>
hipError_t launch_rank_f32(const RankParams& p, dim3 grid, hipStream_t s) {
    constexpr auto kernel = &k_rank_mfma<S::metric, S::TM>;
    if (probe_stage(1, reinterpret_cast<const void*>(kernel), grid, 256, 0, kRankOpsF32)) return hipSuccess;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p.rot, p.cent, p.consts, p.cnorm2, p.nq, p.nlist, p.D, p.scores);
    return hipGetLastError();
}
} // namespace

hipError_t launch_rank_gemm(const RankParams& p, int device, hipStream_t s) {
    const bool wide = p.split && p.wide;
    const uint32_t T = p.big ? 128u : 64u;
    const dim3 grid = wide ? dim3((p.nlist + 255) / 256, (p.nq + 127) / 128)
                           : dim3((p.nlist + T - 1) / T, (p.nq + T - 1) / T, p.split && p.ksplit > 1 ? p.ksplit : 1u); // (z: split-K, the row zeroed by the preparation)
    return with_rank_shape(p.metric, wide, p.big, [&](auto shape) {
        using S = decltype(shape);
        if (p.split && p.f16) return launch_rank_f16<S>(p, grid, device, s);
        if (p.split) return launch_rank_split<S>(p, grid, device, s);
        return launch_rank_f32<S>(p, grid, s);
    });
}

uint32_t select_exact_np2(uint32_t nprobe) { return next_pow2(nprobe); }

hipError_t launch_select_exact(const SelectParams& p, int device, hipStream_t s, uint64_t* key_window) {
    const uint32_t np2 = next_pow2(p.nprobe);
    // key_window != null: [nq][np2] u64 in global memory (nprobe > kNprobeMax)
    const size_t lds = (key_window ? 0 : (size_t)np2 * 8) + (size_t)p.D * 4 + kThreads * 4;
    static LdsAttrCache attr, attr_unf; // nprobe > 4096: more than the default 64 KB of dynamic LDS
    const auto launch = [&](auto kernel, LdsAttrCache& cache) -> hipError_t {
        if (probe_stage(2, reinterpret_cast<const void*>(kernel), dim3(p.nq), kThreads, lds)) return hipSuccess;
        hipError_t e = cache.ensure(reinterpret_cast<const void*>(kernel), lds, device);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(p.nq), dim3(kThreads), lds, s, (const float*)p.scores, p.nlist, p.nprobe, np2, p.metric, p.rot, p.cent,
                           p.D, p.list_gb0, p.list_n, p.probe, p.wl, p.wl_stride, p.nstream, p.nvec, p.prof_total, p.consts, p.bsum, key_window);
        return hipGetLastError();
    };
    return p.numeric_variant == (uint32_t)kVarPortable ? launch(&k_select<true>, attr_unf) : launch(&k_select<false>, attr);
}

namespace {
template <int RM, int V>
hipError_t launch_select_rmv(const SelectParams& p, const SelectGeom& g, size_t lds, int device, hipStream_t s) {
    static LdsAttrCache attr;
    if (probe_stage(2, reinterpret_cast<const void*>(&k_select_mfma<RM, V>), dim3(p.nq), kThreads, lds)) return hipSuccess;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_select_mfma<RM, V>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_select_mfma<RM, V>), dim3(p.nq), dim3(kThreads), lds, s, p, g);
    return hipGetLastError();
}
template <int RM>
hipError_t launch_select_rm(const SelectParams& p, const SelectGeom& g, size_t lds, int device, hipStream_t s) {
    if (p.numeric_variant == (uint32_t)kVarAvx2) return launch_select_rmv<RM, kVarAvx2>(p, g, lds, device, s);
    if (p.numeric_variant == (uint32_t)kVarPortable) return launch_select_rmv<RM, kVarPortable>(p, g, lds, device, s);
    return launch_select_rmv<RM, kVarAvx512>(p, g, lds, device, s);
}
} // namespace

// Static __shared__ of k_select_mfma<RM> (s_todo, s_zone, s_kept ...: 7424 B in the round-3 build), read once from the code
// object: the dynamic-LDS decisions below must leave room for it (with the row in LDS and a 128 KB shortlist
// window, dynamic alone reached 160 KB and the launch failed for n_lists in (6016, 7872] at D = 64).
template <int RM>
size_t select_static_lds() {
    static const size_t v = [] {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_select_mfma<RM>)) != hipSuccess) { (void)hipGetLastError(); return (size_t)8192; }
        return (size_t)fa.sharedSizeBytes;
    }();
    return v;
}

hipError_t launch_select_mfma(const SelectParams& p, int device, hipStream_t s) {
    SelectGeom g;
    g.cap2 = next_pow2(2 * p.nprobe) < 64u ? 64u : next_pow2(2 * p.nprobe);
    const size_t lds0 = (size_t)g.cap2 * 8 + (size_t)p.D * 4 + kThreads * 4;
    // <= 4096 lists: the score row lives in registers; else in LDS while it fits beside the shortlist window AND the
    // kernel's static LDS
    g.row_in_lds = (p.nlist > 4096 && (size_t)p.nlist * 4 <= 65536 &&
                    lds0 + (size_t)p.nlist * 4 + select_static_lds<1>() <= kLdsPerWorkgroupMax) ? 1 : 0;
    size_t lds = lds0 + (g.row_in_lds ? (size_t)p.nlist * 4 : 0);
    g.stage = lds + (size_t)p.nprobe * 16 <= 48 * 1024 ? 1 : 0; // per-probe geometry staged in LDS
    if (g.stage) lds += (size_t)p.nprobe * 16;
    // LDS scorer of the lazy selection: RBQ_SEL_ROWS centroid rows at a time while the workgroup stays below 64 KB (>= 2 per CU)
#ifndef RBQ_SEL_ROWS
#define RBQ_SEL_ROWS 4
#endif
    const size_t rowsN = RBQ_SEL_ROWS * ((size_t)p.D + 8) * 4 + 16;
    g.stage_rows = (p.lazy && lds + rowsN <= 64 * 1024) ? (uint32_t)RBQ_SEL_ROWS : 0u;
    // exact head evaluation (select_mfma.hpp, step 3b): its scratch shares the rows' region (used before the scoring round)
    g.hx_nv = 0;
    size_t regionN = g.stage_rows ? rowsN : 0;
    if (p.lazy && p.head_exact && p.lut && p.top_k <= kHxMaxVec && p.D % 16 == 0) {
#ifndef RBQ_HX_BUDGET
#define RBQ_HX_BUDGET (16384u * 8u)
#endif
        uint32_t nv = (uint32_t)(((uint32_t)RBQ_HX_BUDGET / p.Dc) / 32u * 32u); // vectors evaluated: ~128 K code dimensions per query
        nv = nv < 64u ? 64u : (nv > kHxMaxVec ? kHxMaxVec : nv);
        const size_t hxN = (hx_scratch_bytes(p.D, p.Dc, p.ex_bits, nv) + 15) & ~(size_t)15;
        if (lds + std::max(regionN, hxN) <= 64 * 1024) { g.hx_nv = nv; regionN = std::max(regionN, hxN); }
    }
    lds += regionN;
    g.cand_cap = (uint32_t)(((g.stage ? (size_t)p.nprobe * 16 : 0) + (g.stage_rows ? rowsN - 16 : 0)) / 8); // (RM == 0 prefilter window)
    if (p.nlist <= 4096) return launch_select_rm<2>(p, g, lds, device, s);
    if (g.row_in_lds) return launch_select_rm<1>(p, g, lds, device, s);
    return launch_select_rm<0>(p, g, lds, device, s);
}

hipError_t launch_probes_given(const ProbesGivenParams& p, hipStream_t s) {
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(p.nq), dim3(kThreads), (size_t)p.D * 4 + kThreads * 4, s, p.list_ids, p.list_counts, p.max_lists,
                           p.nlist, p.metric, p.rot, p.cent, p.D, p.list_gb0, p.list_n, p.probe, p.wl, p.wl_stride, p.nstream, p.consts, p.bsum);
    };
    if (p.numeric_variant == (uint32_t)kVarPortable) launch(&k_probes_given<true>);
    else launch(&k_probes_given<false>);
    return hipGetLastError();
}

} // namespace rbq
