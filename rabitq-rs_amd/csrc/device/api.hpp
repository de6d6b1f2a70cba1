// api.hpp — internal header of librbq.so's host side: the C ABI of include/rbq.h over the HIP kernels, which the host
// units (api_index, api_build, api_append, api_remove, api_search, api_mstg_search, api_save, api_load, api_fetch, api_bf, api_bf_mutate, api_mstg, api_mstg_mutate, api_mstg_persist) reach through launch.hpp.  Not installed.
// Host responsibilities: validate like the reference (src/ivf.rs:1754-1769,1484-1702), upload the reference's ClusterData
// bytes and have the GPU re-lay them into the device layout (one-time, at create/load), own HBM on one or N devices
// (replicas), and enqueue prep -> rank -> select -> scan for each query batch.  There is no CPU compute path: every failure
// to reach the GPU surfaces as RBQ_DEVICE.  Everything declared here is hidden: only the units' extern "C" entry points
// enter the dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "rbq.h"
#include "launch.hpp"
#include "../host/rbq_host_logic.hpp"
#include "../host/rbq_index_layout.hpp"
#include "../host/rbq_append_plan.hpp"
#include "../host/rbq_search_plan.hpp"

#pragma GCC visibility push(hidden)

namespace rbq_api {

using namespace rbq;
using rbq_host::ListSrc;
using rbq_host::OutPack;
using rbq_host::align_up;

inline thread_local std::string g_err;

inline int fail(int code, const std::string& detail) {
    g_err = detail;
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess)                                                                       \
            return fail(RBQ_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

// No C++ exception may cross the C boundary (the Rust host is panic = "abort", Cargo.toml:59; ctypes would
// terminate): every entry point runs inside this guard.
#define RBQ_GUARD_BEGIN try {
#define RBQ_GUARD_END                                                                               \
    } catch (const std::bad_alloc&) { return fail(RBQ_IO, "out of host memory"); }                 \
    catch (const std::exception& e) { return fail(RBQ_IO, std::string("internal error: ") + e.what()); } \
    catch (...) { return fail(RBQ_IO, "internal error"); }

// Entry points switch to the index's device and put the caller's device back on exit.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Busy-waits (with the CPU's pause hint) until pred() holds or `limit` has passed; returns pred()'s last value.
template <class Pred>
bool spin_until(Pred pred, std::chrono::microseconds limit = std::chrono::microseconds::max()) {
    const bool timed = limit != std::chrono::microseconds::max();
    const auto t0 = timed ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    while (!pred()) {
        if (timed && std::chrono::steady_clock::now() - t0 >= limit) return false;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return true;
}

// Whether a caller's buffer lives in device memory (else it is treated as host memory and copied)
inline bool is_device_pointer(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice;
}

// rescale: RBQ_RESCALE_CONST (t_const for every vector) or RBQ_RESCALE_OPTIMAL (k_rescale per vector; t_const ignored).
// Returns whether the per-vector search runs (it is moot for 1-bit indexes), or -1 after fail() for an unknown mode.
inline int rescale_mode(int rescale, const rbq_header* hdr) {
    if (rescale != RBQ_RESCALE_CONST && rescale != RBQ_RESCALE_OPTIMAL) {
        fail(RBQ_INVALID_CONFIG, "unknown rescale mode " + std::to_string(rescale) + " (RBQ_RESCALE_CONST or RBQ_RESCALE_OPTIMAL)");
        return -1;
    }
    return rescale == RBQ_RESCALE_OPTIMAL && hdr && hdr->ex_bits > 0 ? 1 : 0;
}

// A growing scratch buffer in device memory, or (Pinned) in page-locked host memory, freed with its owner.  The owner
// destroys it under its DeviceGuard.
template <bool Pinned>
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return RBQ_OK;
        release();
        const size_t want = bytes + bytes / 8 + (Pinned ? 4096 : 256);
        if constexpr (Pinned) HIP_TRY(hipHostMalloc(&p, want, hipHostMallocPortable)); // portable: mapped for every device, not only the current one
        else HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return RBQ_OK;
    }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
};
using DevBuf = Buf<false>;
using PinBuf = Buf<true>; // page-locked host staging

// What one call allocates for itself (device and page-locked memory, events, a private stream), freed on every exit.
// The stream is drained before anything is freed: work still queued on it may read or write the allocations.
struct Scratch {
    hipStream_t stream = nullptr;
    std::vector<void*> dev, pin;
    std::vector<hipEvent_t> events;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void* p : pin) (void)hipHostFree(p);
        for (void* p : dev) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    hipError_t make_stream() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
    template <class T> hipError_t alloc(T** p, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) { dev.push_back(q); *p = (T*)q; }
        return e;
    }
    template <class T> hipError_t alloc_pinned(T** p, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipHostMalloc(&q, bytes ? bytes : 16, hipHostMallocDefault);
        if (e == hipSuccess) { pin.push_back(q); *p = (T*)q; }
        return e;
    }
    hipError_t event(hipEvent_t* ev) {
        const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
};

// Persistent host threads that run posted jobs (Job: a callable), started once and joined by shutdown().  A thread that
// has just finished a job polls ~100 us for the next one before it blocks: callers that post back to back find it hot.
template <class Job, int kThreads>
struct WorkerPool {
    std::thread th[kThreads];
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> jobs;
    std::atomic<uint32_t> pending{0};
    bool stop = false;
    void run() {
        for (;;) {
            Job job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [this] { return stop || !jobs.empty(); });
                if (jobs.empty()) return; // stop requested and nothing left
                job = std::move(jobs.front());
                jobs.pop_front();
            }
            job();
            pending.fetch_sub(1, std::memory_order_release);
            (void)spin_until([this] { return pending.load(std::memory_order_acquire) != 0; }, std::chrono::microseconds(100));
        }
    }
    // false: a thread could not be created (the ones that did start are shut down again).  A pool is published only once
    // start() has returned true: jobs posted to a half-started pool could wait forever.
    bool start() {
        try {
            for (auto& t : th) t = std::thread([this] { run(); });
        } catch (...) {
            shutdown();
            return false;
        }
        return true;
    }
    void post(Job j) {
        pending.fetch_add(1, std::memory_order_release);
        { std::lock_guard<std::mutex> lk(mu); jobs.push_back(std::move(j)); }
        cv.notify_one();
    }
    void shutdown() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto& t : th) if (t.joinable()) t.join();
    }
};

// Persistent staging helpers of a replica (rbq_search_batch with PAGEABLE queries).  The queries of a call must be copied once
// into page-locked memory before the GPU can read them; one thread copies 3.9 MB (1024 x 960 f32) in ~165 us — more than half of the
// ~280 us the same call takes from page-locked buffers.  The sub-batches of a call have their own lanes and staging buffers, so
// their copies are independent: the caller copies sub-batch 0 (and launches it at once), the helpers copy the others meanwhile.
// Started on the first pageable call, joined when the replica is freed.
struct StageJob {
    void* dst = nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
    std::atomic<int>* done = nullptr;
    void operator()() const {
        std::memcpy(dst, src, bytes);
        done->store(1, std::memory_order_release);
    }
};
using StagePool = WorkerPool<StageJob, 3>;

// Persistent host threads per replica beyond the first (rbq_search_batch on N replicas): the shard of replica r is
// enqueued and awaited by a worker of replica r while the caller's own thread serves replica 0.  Started on the first
// multi-replica call, joined when the index is destroyed — no thread is created per call (8 replicas: seven thread start-ups
// of 30-50 us each per call were as long as a 1024-query shard itself).  Two threads per replica, so that the shards of two
// concurrent callers overlap on it.
using ReplicaPool = WorkerPool<std::function<void()>, 2>;

struct Workspace {
    hipStream_t stream = nullptr;
    DevBuf queries, rot, lut, consts, scores, probe, wl, nstream, nvec, out_pack, filter, rot_hl, rank_planes, dead_skipped, heap_ws, key_window, audit_dead, tie_log, head_ub;
    // rot_hl: the split-bf16 image of the rotated queries, hi | lo interleaved per K slab (hl_layout.hpp); rank_planes: planar
    // copies of both GEMM operands (debug option rank_planar)
    DevBuf rot_f16, rank_resid; // one-product f16 route: the f16 image [nq][D] of the rotated queries and |q - f16(q)| per query
    DevBuf ms_sl, ms_lists; // rbq_mstg_search_batch*: shortlists | their lengths | query norms; the selected lists | their counts
    DevBuf mr_pool;         // rbq_mstg_search_refined_batch*: the pool's slots [n][pool] u64 | estimates [n][pool] f32 | counts [n] u32
    DevBuf rr_ids, rr_est, rr_counts; // pooled rerank: the pool's ids [n][pool] u64, estimates [n][pool] f32, counts [n] u32
    PinBuf h_in, h_out;      // rbq_search_batch: staging of one sub-batch
    hipEvent_t done = nullptr; // results of the sub-batch in flight have reached h_out / the caller's buffers
    uint64_t call_nq = 0;       // queries of the WHOLE host call this launch chain belongs to (0: a device-entry call — its own nq counts)
    bool latency_first = false; // this launch chain belongs to a host call that waits for it (rbq_search_batch below kHostWaveMinQueries)
    Workspace() = default;
    Workspace(const Workspace&) = delete;
    ~Workspace() { // (deleted under the owner's DeviceGuard)
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct StageProf {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; // pairs recorded since rbq_profile_begin
    double ms = 0;
    uint64_t launches = 0;
    std::vector<float> samples; // duration of every timed launch, in launch order
};
// Event pairs are created once and recycled: hipEventCreate inside the launch path cost ~15 % of the
// overlapped throughput and broke down beyond three caller streams.
struct EventPool {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_pairs;
    bool take(std::pair<hipEvent_t, hipEvent_t>& p) {
        if (!free_pairs.empty()) { p = free_pairs.back(); free_pairs.pop_back(); return true; }
        // timing only: without the system-scope fence a default event performs when it completes (that fence sits
        // between the kernels of a stream and shows up in the overlapped throughput)
        if (hipEventCreateWithFlags(&p.first, hipEventDisableSystemFence) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&p.second, hipEventDisableSystemFence) != hipSuccess) { (void)hipEventDestroy(p.first); return false; }
        return true;
    }
    void give(const std::pair<hipEvent_t, hipEvent_t>& p) { free_pairs.push_back(p); }
    void destroy() {
        for (auto& e : free_pairs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        free_pairs.clear();
    }
};

struct Arr { // one device array of a replica (size kept for cloning)
    void* p = nullptr;
    size_t bytes = 0;
};

// What an index's header fixes about its vectors and queries (IVF replicas and the brute-force index alike).
struct Geometry {
    uint32_t dim = 0, D = 0, Dc = 0; // dimension, padded dimension, padded dimension rounded up to 64 (code blocks)
    uint8_t metric = 0, rotator = 0, ex_bits = 0;
    uint32_t trunc = 0; // the FHT rotator's length: the largest power of two <= dim
    float fac = 1.0f;   // 1 / sqrt(trunc)
};
inline Geometry geometry_of(const rbq_header& h) {
    Geometry g;
    g.dim = h.dim; g.D = h.padded_dim; g.Dc = (h.padded_dim + 63u) / 64u * 64u;
    g.metric = h.metric; g.rotator = h.rotator; g.ex_bits = h.ex_bits;
    uint32_t lg = 0;
    for (uint32_t x = h.dim; x >>= 1;) ++lg;
    g.trunc = 1u << lg;
    g.fac = 1.0f / std::sqrt((float)g.trunc);
    return g;
}

// k_prep's parameters for nq queries at `queries` (device-visible): the index's geometry and rotator, the workspace's
// rot / lut / consts (both workspace types name them alike).  No split-bf16 copies, one wave per query.
// query_dtype: RBQ_RAW_* of the rows at `queries` (the option "query_dtype" of an IVF / MSTG handle; the brute-force index: f32).
template <class Ws>
PrepParams prep_params(const Geometry& g, const Arr& rot_blob, Ws& w, const void* queries, uint64_t nq, int query_dtype = kRawF32) {
    PrepParams p;
    p.queries = queries; p.query_dtype = query_dtype; p.nq = (uint32_t)nq; p.dim = g.dim; p.D = g.D; p.Dc = g.Dc; p.rotator = (int)g.rotator;
    p.rot_blob = (const uint8_t*)rot_blob.p; p.trunc = g.trunc; p.fac = g.fac; p.ex_bits = g.ex_bits;
    p.rot = (float*)w.rot.p; p.lut = (uint8_t*)w.lut.p; p.consts = (QueryConsts*)w.consts.p;
    p.rot_hl = nullptr; p.wg_prep = false;
    return p;
}

// Default of the `scan_wave` option; RBQ_SCAN_WAVE=0|1|2 in the environment overrides it (A/B runs of the whole test suite).
inline int scan_wave_default() {
    static const int v = [] { const char* e = std::getenv("RBQ_SCAN_WAVE"); return e && *e ? std::atoi(e) : 2; }();
    return v;
}

// Per-index settings (rbq_debug_set_option, rbq_index_set_numeric_variant), each with its default.  Every replica holds the
// same values.
struct Options {
    uint32_t numeric_variant = 0; // RBQ_NUMERIC_*: which build of the reference the kernels reproduce (kernels.hpp, kVar*)
    uint32_t host_lanes = 0, host_subbatch = 0, host_trace = 0; // pipeline shape of rbq_search_batch (0 = default)
    int rank_ksplit = 1;          // 0 = never split the ranking GEMM's K loop, 1 = by batch size, n > 1 = forced (min(n, 4) parts)
    bool host_zero_copy = true;   // rbq_search_batch: k_prep reads the queries from page-locked host memory in place (no H2D copy command)
    bool host_stage_helpers = true; // rbq_search_batch: pageable queries of a call's later sub-batches are staged by helper threads
    bool no_block_bound = false, f32_rank = false, wg_prep = false, exact_heap = false, force_rank_fallback = false, exact_rank = false;
    bool head_exact = true;  // lazy selection: a bound of the k-th distance from real estimates of the nearest list's first vectors
    bool lazy_filter = true; // search_filtered: lazy selection on the exact head evaluation's bound (filter-passing vectors only)
    bool lazy_fault_inject = false; // TEST ONLY: makes the lazy selection wrong on purpose (tests/test_gpu_round4.py: the audit must notice)
    SlackMul slack;          // TEST ONLY (options slack_term / slack_milli): multipliers of block_ub()'s rounding-slack terms
    int slack_term = 0;
    bool ub_tap = false;     // DIAGNOSTIC: the select kernel exports its head bounds (workspace "head_ub")
    bool lazy_audit = false; // DIAGNOSTIC: the select kernel exports the lists it drops as a whole (workspace "audit_dead")
    bool lazy_select = true; // probe selection drops lists that are provably skipped as a whole (select_mfma.hpp)
    uint32_t tie_log_cap = 0; // TEST ONLY: entries per query of the tie log (0 = the default sizes)
    bool tie_log = true;      // k_scan logs the candidates it refines; a tied query replays the log (topk.hpp)
    int latency_path = 1;     // small calls (see kLatMaxQueries) take the latency-first front (latency.hpp); 0 = never
    int rank_tile = 0;        // tile of the split-bf16 ranking GEMM (0 = by problem size)
    int rank_f16 = -1;        // one-product f16 ranking GEMM: -1 = by rule (big or wide calls at D >= 256), 0 = never, 1 = whenever possible
    bool rank_planar = false; // TEST ONLY: the split-bf16 ranking GEMM reads planar copies of its operands (de-interleaved per call)
    uint32_t stage_mask = 0xf; // DIAGNOSTIC: bit s = launch stage s (prep, rank, select, scan); a skipped stage leaves the workspace
                               // of the stream as the last full call wrote it — results are then those of THAT batch (rate probes only)
    int scan_wave = scan_wave_default(); // which scan kernel serves a call: 0 = k_scan (one workgroup per query), 1 = k_scanw (one wave per
                                         // query) wherever it serves the call shape, 2 = by batch size (kScanWaveMinQueries)
    bool profile_counters = true; // an open profile keeps the traffic counters (0: stage timings only — the counters cost the
                                  // pipelined run 2-3 %, bench.py collects them in a pass of their own)
    uint64_t save_chunk = 0;  // TEST ONLY: staging chunk of rbq_index_save_rbq1_stream in bytes (0 = default)
    uint64_t fetch_chunk = 0; // TEST ONLY: ids per staging chunk of rbq_index_fetch_embeddings (0 = default)
    uint64_t mstg_chunk = 0;  // TEST ONLY: staging chunk of rbq_mstg_save* in bytes, any value >= 1 (0 = default)
    uint64_t mstg_search_budget = 0; // TEST ONLY: per-chunk workspace of rbq_mstg_search_batch* in bytes (0 = default)
    int query_dtype = 0;      // RBQ_RAW_*: what every entry point that takes queries reads its pointer as (0: f32)
    int rerank_raw_dtype = 0; // RBQ_RAW_*: the element type the next rbq_index_set_rerank_vectors reads its pointer as (0: f32)
    uint32_t rerank_pool = 0; // while rerank is on and rerank_pool > top_k: the search runs at top_k := rerank_pool, the pool is scored
                              // exactly against the attached vectors and the best top_k are returned (0 = off; <= kRerankPoolMax)
    bool mstg_rerank = false; // rbq_mstg_search_refined_batch* only: the pool is reduced to one entry per id and
                              // scored exactly against the attached raw vectors instead of the ex codes (needs vectors attached, rerank 1)
    // range search: while range_search is on, rbq_search_batch / rbq_search_batch_device return every probed
    // vector whose distance is below the radius (an f32 passed by its bits; distance < r for L2, score > r for inner product), in
    // scan order, with top_k read as the capacity of the output row and out_counts as the total
    bool range_search = false;
    uint32_t range_radius_bits = 0x7f800000u; // +inf
    // exact range search: while range_search and range_exact are on (raw vectors attached, rerank 1), the
    // matches of the estimate at range_radius_bits are only candidates; each is scored exactly against its raw row and kept iff
    // exact distance < x (L2) or exact dot product > x (inner product), x the f32 of these bits
    bool range_exact = false;
    uint32_t range_exact_radius_bits = 0x7f800000u; // +inf
    // option `name` := value (the options of rbq_debug_set_option that live in Options); RBQ_INVALID_CONFIG for an unknown name
    int set(const char* name, int value);
};

// The option fields the search routing reads (rbq_host::plan_search): THE place where Options meets the plan.
inline rbq_host::RouteOptions route_options(const Options& o) {
    rbq_host::RouteOptions r;
    r.exact_rank = o.exact_rank; r.f32_rank = o.f32_rank; r.wg_prep = o.wg_prep; r.latency_path = o.latency_path;
    r.rank_ksplit = o.rank_ksplit; r.rank_tile = o.rank_tile; r.rank_f16 = o.rank_f16; r.rank_planar = o.rank_planar;
    r.stage_mask = o.stage_mask; r.lazy_select = o.lazy_select; r.lazy_filter = o.lazy_filter; r.head_exact = o.head_exact;
    r.no_block_bound = o.no_block_bound; r.scan_wave = o.scan_wave; r.tie_log = o.tie_log; r.tie_log_cap = o.tie_log_cap;
    r.exact_heap = o.exact_heap;
    return r;
}

// One device-resident copy of the index.
struct Replica : Geometry {
    int device = 0;
    uint64_t n_vectors = 0, n_lists = 0, n_blocks = 0;
    Arr rot_blob, centroids, blocks, ids, ex, fadd_ex, fres_ex, list_gb0, list_n, prof, bsum, cnorm2, fallbacks, cent_hl, raw,
        bsumx, lsum, // ex-factor ranges per block, factor ranges per list (lazy probe selection)
        cent_f16, cent_f16_resid; // one-product f16 image [nlist][D] of the centroids and |c - f16(c)| per centroid (rank_mfma.hpp header)
    // reconstruction factors delta / vl of every slot (RBQ1's per-vector arrays that search never reads): kept on the FIRST
    // replica only, for rbq_index_save_rbq1 (clone_replica does not copy them)
    Arr delta, vl;
    // MSTG handles only (rbq_mstg_build_device, rbq_mstg_load*; FIRST replica, slot order, pad slots 0): QuantizedVector::residual_norm,
    // which the `.mstg` format stores and no search reads — 4 bytes per vector — and the RabitqConfig::t_const the lists were built with
    Arr rnorm;
    bool has_rnorm = false, tc_some = false;
    float tc_value = 0.0f;
    bool has_recon = false; // false: created by rbq_index_create (no factors given) — such a handle cannot be saved
    // fetch_embedding's id map (FIRST replica only): every vector's id, ascending (stably sorted: the first (cluster, position)
    // occurrence first), and its slot — 12 bytes per vector, built by the first fetch under fetch_mu, kept until destroy
    std::mutex fetch_mu;
    Arr fmap_ids, fmap_slots;
    bool fmap_ready = false;
    // rbq_mstg_search_batch*: split-bf16 images of the centroids (padded to 32), their norms | largest norm | non-finite flag; built
    // by the first search that takes the GEMM shortlist, under `mu`, kept until destroy (built per replica)
    Arr ms_hi, ms_lo, ms_nc;
    bool ms_ready = false;
    uint32_t ms_bad = 0;
    // rbq_mstg_search_refined_batch*: the identity slot map the scan reports positions through (8 bytes per slot) and the list of
    // every block; built by the first refined search, under `mu`, kept until destroy (built per replica)
    Arr mr_slot_map, mr_blk_list;
    bool mr_ready = false;
    // THE list of the device arrays a replica owns (free_replica, rbq_mstg_memory_usage): the first kCloned are what clone_replica
    // copies (`raw` excepted), the others stay with the replica that built them
    static constexpr size_t kCloned = 19;
    Arr* arrays[29] = {&rot_blob, &centroids, &blocks, &ids, &ex, &fadd_ex, &fres_ex, &list_gb0, &list_n, &prof, &bsum, &cnorm2,
                       &fallbacks, &cent_hl, &raw, &bsumx, &lsum, &cent_f16, &cent_f16_resid,
                       &delta, &vl, &rnorm, &fmap_ids, &fmap_slots, &ms_hi, &ms_lo, &ms_nc, &mr_slot_map, &mr_blk_list};
    float cnorm2_max = 0.0f;
    // one-product f16 ranking: sqrt(cnorm2_max) and the largest |c - f16(c)|, both rounded up; rank_f16_ok: every stored half is
    // finite and rc_max <= 2^-11 cnorm_max (else the index ranks on split-bf16 for good)
    float cnorm_max = 0.0f, rc_max = 0.0f;
    bool rank_f16_ok = false;
    uint64_t n_raw = 0;      // raw vectors attached for the optional rerank
    int raw_dtype = 0;       // RBQ_RAW_* of the attached rows (kRawF32 while nothing is attached)
    bool raw_borrowed = false;
    bool rerank = false;
    Options opt;
    std::unique_ptr<StagePool> stagers; // (created on the first pageable call, under `mu`; published only when all its threads run)
    bool stagers_failed = false;        // thread creation failed once: pageable calls stage inline from then on
    // host
    std::vector<uint32_t> h_list_n;
    std::vector<uint64_t> nblk_desc_prefix; // prefix sums of per-list block counts sorted descending
    std::mutex mu;
    std::vector<Workspace*> pool;
    std::map<hipStream_t, Workspace*> stream_ws; // stream_workspace(): one workspace per caller stream
    // profiling
    bool profiling = false;
    uint32_t prof_mask = 0xf; // stages that are timed while `profiling` (bit s = stage s)
    uint32_t prof_every = 1;  // time every n-th launch of a stage
    uint32_t prof_seq[4] = {0, 0, 0, 0};
    StageProf stage_prof[4]; // prep, rank, select, scan
    EventPool ev_pool;
    uint64_t prof_counters[kProfSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
    // rbq_index_id_bound (FIRST replica only): 1 + the largest stored id, found by one reduction over `ids` on first use, under
    // idb_mu, kept until destroy (rbq_index_append sets it for the handle it returns)
    std::mutex idb_mu;
    uint64_t id_bound = 0;
    bool idb_ready = false;
    Replica() = default;
    Replica(const Replica&) = delete;
};

// The byte size of every array of a replica (csrc/host/rbq_index_layout.hpp)
static_assert(sizeof(BlockSummary) == rbq_host::kBlockSummaryBytes && sizeof(BlockSummaryEx) == rbq_host::kBlockSummaryBytes,
              "index_bytes() sizes bsum, bsumx and lsum");
inline rbq_host::IndexBytes index_bytes_of(const Replica* ix) {
    return rbq_host::index_bytes(ix->D, ix->Dc, ix->ex_bits, ix->n_blocks, ix->n_lists);
}

// shared by the units (api_index.hip)
int alloc_arr(Arr& a, size_t bytes);
int upload_arr(Arr& a, const void* src, size_t bytes);
void free_replica(Replica* ix);
struct ReplicaOwner { // frees a half-built replica on an early return
    Replica* ix;
    ~ReplicaOwner() { if (ix) free_replica(ix); }
    Replica* release() { Replica* r = ix; ix = nullptr; return r; }
};
int validate_header(const rbq_header* h, bool brute_force = false);
int resolve_devices(int n_devices, const int* devices, std::vector<int>& out);
Replica* new_replica(const rbq_header* hdr, int dev);
// THE allocation of a replica's slot and block arrays, shared by every construction path: sets n_blocks, n_vectors, has_recon and
// has_rnorm, uploads list_gb0 / list_n, allocates blocks, ids, ex, fadd_ex, fres_ex, bsum (delta and vl with `recon`, rnorm with
// `rnorm`) at index_bytes' sizes and zeroes the read-ahead pad of `ex`.  rot_blob, centroids, a path's own fills and tc_some /
// tc_value stay with the caller.
int alloc_index_arrays(Replica* ix, const std::vector<uint32_t>& ln, const std::vector<uint32_t>& gb0, uint64_t n_blocks,
                       uint64_t n_vectors, bool recon, bool rnorm);
int finish_replica(Replica* ix, const std::vector<uint32_t>& ln);
int wrap_and_replicate(Replica* first, const std::vector<int>& devs, rbq_index** out);
// api_build.hip: the device encoder over (vector, list) pairs (rbq_index_build_device_ex: one pair per vector; rbq_mstg_build_device)
int build_device_pairs(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                       const uint32_t* d_vec, uint64_t n, int rescale, float t_const, int dev, rbq_index** out);

// api_build.hip: what the streamed builder and rbq_index_append share.  encode_rows_at_cursors rotates, encodes and scatters n
// device-resident rows (ids id_base + row) into the slots their lists' cursors point at, advances the cursors and returns once
// the device is idle (the scratch, and a caller's staging buffers, may be reused).  d_block_list: the list of every block;
// d_cursor [n_lists]: vectors each list holds so far; d_chunk_first [n_lists]: scratch.
// d_pair_row (rbq_mstg_append; null: row j is pair j): the n entries are (row, list) PAIRS in ascending row order, pair j stores row
// d_pair_row[j] of d_vec in list d_asg[j] under the id id_base + d_pair_row[j]: several slots share one source row and one id.
// A replica with `rnorm` gets the residual norm of every slot written too.
struct EncodeScratch { DevBuf vec, assign, ko, vi, vo, tmp, row_src, row_slot, rows, raw, trow; };
int encode_rows_at_cursors(Replica* ix, EncodeScratch& sc, const float* d_vec, const uint32_t* d_asg, uint32_t n, uint64_t id_base,
                           bool opt, float t_const, const uint32_t* d_block_list, uint32_t* d_cursor, uint32_t* d_chunk_first,
                           const uint32_t* d_pair_row = nullptr);
// rows per encode chunk: the 512 MiB budget of the rotated rows
inline uint64_t encode_chunk_rows(uint32_t D) { return std::max<uint64_t>(1024, ((512ull << 20) / ((size_t)D * 4)) & ~63ull); }
// block -> list and block -> number of real vectors, on the device
int upload_block_tables(const std::vector<uint32_t>& ln, const std::vector<uint32_t>& gb0, uint64_t nblocks, Scratch& t,
                        uint32_t** d_block_list, uint32_t** d_block_nv);

// what rbq_index_append and rbq_index_remove_ids (api_append.hip, api_remove.hip) share
struct EventPair { // times one launch on the null stream; freed on every exit
    hipEvent_t a = nullptr, b = nullptr;
    bool ok = false;
    EventPair() {
        ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
        if (!ok) (void)hipGetLastError();
    }
    EventPair(const EventPair&) = delete;
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void start() { if (ok) ok = hipEventRecord(a, 0) == hipSuccess; }
    void stop() { if (ok) ok = hipEventRecord(b, 0) == hipSuccess; }
    bool ns(uint64_t* out) {
        float ms = 0.0f;
        if (!ok || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return false; }
        *out = (uint64_t)((double)ms * 1e6);
        return true;
    }
};

// the per-slot arrays of a replica for the carry / gather kernels (null where it holds none)
inline SlotArrays slot_arrays(const Replica* ix) {
    SlotArrays a{};
    a.blocks = (uint8_t*)ix->blocks.p; a.ids = (uint64_t*)ix->ids.p; a.delta = (float*)ix->delta.p; a.vl = (float*)ix->vl.p;
    if (ix->ex_bits) { a.ex = (uint8_t*)ix->ex.p; a.fadd = (float*)ix->fadd_ex.p; a.fres = (float*)ix->fres_ex.p; }
    if (ix->has_rnorm) a.rnorm = (float*)ix->rnorm.p;
    return a;
}
// What rbq_index_append and rbq_mstg_append share (api_append.hip): the replica of the grown geometry — centroids and rotator bit
// for bit those of `old`, every array allocated (rnorm too where `old` has it), the old arrays carried over by k_append_carry — and
// its block tables in `t`.  own.ix is the new replica (freed by `own` on an early return).
int append_grow(Replica* old, const rbq_host::AppendPlan& plan, Scratch& t, ReplicaOwner& own, uint32_t** d_block_list,
                uint32_t** d_block_nv);
// What rbq_index_remove_ids and rbq_mstg_remove_ids share (api_remove.hip): everything after the argument checks.  A handle with
// `rnorm` (an MSTG handle) has it gathered with the other slot arrays and hands on tc_some / tc_value.
int remove_ids_core(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, const std::vector<int>& devs, uint64_t* out_removed,
                    rbq_index** out);
// api_mstg.hip: closure_device with the argument's memories detected; `count` adds its fallbacks to rbq_mstg_debug_closure_fallbacks
int run_closure(ClosureArgs& a, int dev, bool count);
// 1 + the largest stored id of a handle's first replica, computed once (api_append.hip)
int id_bound_of(Replica* ix, uint64_t* out);

// shared by the search units (api_search.hip): workspaces from the replica's pool and per caller stream, the stage timer, the scan launch
Workspace* take_ws(Replica* ix);
void give_ws(Replica* ix, Workspace* w);
Workspace* stream_workspace(Replica* ix, hipStream_t s);
int check_query_args(const rbq_index* h, uint32_t query_dim);
// the handle's query rows (option "query_dtype") of `query_dim` elements; check_query_pointer: RBQ_INVALID_CONFIG for a pointer that
// cannot hold them (16-bit rows at an odd address) — no HIP call is made to find out
inline rbq_host::QueryRows query_rows(const Replica* ix, uint32_t query_dim) { return rbq_host::QueryRows{ix->opt.query_dtype, query_dim}; }
int check_query_pointer(const rbq_index* h, const void* queries);
Replica* replica_of_pointer(rbq_index* h, const void* dptr);
struct ProfScope {
    Replica* ix; int stage; hipStream_t s; std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    bool on = false, ext = false;
    // ext: the launch itself carries the event pair (hipExtLaunchKernelGGL: start/stop come from the dispatch
    // packet, no separate marker packets in the queue); otherwise the pair is recorded around the scope
    ProfScope(Replica* ix_, int st, hipStream_t s_, bool ext_ = false) : ix(ix_), stage(st), s(s_), ext(ext_) {
        if (ix->profiling && !stage_probes() && ((ix->prof_mask >> st) & 1u)) { // (a probed call launches nothing: no event pair for it)
            {
                std::lock_guard<std::mutex> g(ix->mu);
                if (ix->prof_seq[st]++ % ix->prof_every == 0) on = ix->ev_pool.take(ev);
            }
            if (on && !ext) (void)hipEventRecord(ev.first, s);
        }
    }
    hipEvent_t start() const { return on && ext ? ev.first : nullptr; }
    hipEvent_t stop() const { return on && ext ? ev.second : nullptr; }
    ~ProfScope() {
        if (on) {
            if (!ext) (void)hipEventRecord(ev.second, s);
            std::lock_guard<std::mutex> g(ix->mu);
            ix->stage_prof[stage].ev.push_back(ev);
        }
    }
};
// The routing plan of one launch chain of nq queries on workspace w (rbq_search_plan.hpp).  mstg: the posting scan behind the MSTG
// front (nprobe: the list stride; only the plan's scan part is read).
rbq_host::SearchPlan search_plan(const Replica* ix, const Workspace* w, uint64_t nq, uint32_t top_k, uint32_t nprobe, bool has_filter,
                                 bool has_diag, bool range, bool mstg);
// (plan: which scan kernel, the tie log, where the heap lives.  mstg, d_slot_ids: the MSTG scans; the IVF search passes no slot map)
int scan_stage(Replica* ix, Workspace* w, const rbq_host::SearchPlan& plan, uint64_t nq, uint32_t probe_stride, uint32_t top_k,
               uint64_t wl_stride, const uint32_t* d_filter, uint64_t filter_nbits, uint64_t* d_ids, float* d_scores, uint32_t* d_counts,
               rbq_diag* d_diag, bool mstg, const uint32_t* d_dead_skipped, hipStream_t stream, const uint64_t* d_slot_ids = nullptr);

} // namespace rbq_api

struct rbq_index {
    std::vector<rbq_api::Replica*> reps; // reps[r] lives on device reps[r]->device; all hold the same index
    int debug_replica = 0;               // which replica the rbq_debug_copy_* calls read
    std::mutex worker_mu;
    std::vector<std::unique_ptr<rbq_api::ReplicaPool>> workers; // workers[r - 1] serves replica r (created on first use)
};

#pragma GCC visibility pop
