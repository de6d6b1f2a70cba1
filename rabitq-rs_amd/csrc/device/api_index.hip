// api_index.hip — index handles: create / load / clone / destroy, header validation, rerank vectors, host allocation,
// error strings and ABI version, numeric variant, options, profiling, debug counters and copies.
#include "api.hpp"

using namespace rbq_api;

// The HIP runtime multiplexes a process's streams over its hardware queues; the queue count is a process-wide setting of the host
// (GPU_MAX_HW_QUEUES, read when the runtime initialises) and the library leaves it alone.  rbq_process_defaults() used to raise it;
// more queues than a card's slots is a state that has hung shared machines, so it now changes nothing and is kept for the ABI.
extern "C" int rbq_process_defaults(void) {
    return RBQ_OK;
}

namespace rbq_api {
int alloc_arr(Arr& a, size_t bytes) {
    HIP_TRY(hipMalloc(&a.p, bytes ? bytes : 16));
    a.bytes = bytes;
    return RBQ_OK;
}
int upload_arr(Arr& a, const void* src, size_t bytes) {
    int rc = alloc_arr(a, bytes);
    if (rc) return rc;
    if (bytes) HIP_TRY(hipMemcpy(a.p, src, bytes, hipMemcpyHostToDevice));
    return RBQ_OK;
}

int alloc_index_arrays(Replica* ix, const std::vector<uint32_t>& ln, const std::vector<uint32_t>& gb0, uint64_t n_blocks,
                       uint64_t n_vectors, bool recon, bool rnorm) {
    ix->n_blocks = n_blocks; ix->n_vectors = n_vectors; ix->has_recon = recon; ix->has_rnorm = rnorm;
    const rbq_host::IndexBytes B = index_bytes_of(ix);
    int rc;
    if ((rc = upload_arr(ix->list_gb0, gb0.data(), B.list_gb0))) return rc;
    if ((rc = upload_arr(ix->list_n, ln.data(), B.list_n))) return rc;
    if ((rc = alloc_arr(ix->blocks, B.blocks))) return rc;
    if ((rc = alloc_arr(ix->ids, B.ids))) return rc;
    if ((rc = alloc_arr(ix->ex, B.ex_alloc))) return rc;
    if ((rc = alloc_arr(ix->fadd_ex, B.fadd_ex))) return rc;
    if ((rc = alloc_arr(ix->fres_ex, B.fres_ex))) return rc;
    if ((rc = alloc_arr(ix->bsum, B.bsum))) return rc;
    if (recon && ((rc = alloc_arr(ix->delta, B.delta)) || (rc = alloc_arr(ix->vl, B.vl)))) return rc;
    if (rnorm && (rc = alloc_arr(ix->rnorm, B.rnorm))) return rc;
    if (B.ex_alloc) HIP_TRY(hipMemset((uint8_t*)ix->ex.p + B.ex, 0, rbq_host::kExReadAhead)); // read-ahead pad of the refine loads
    return RBQ_OK;
}

void free_replica(Replica* ix) {
    if (!ix) return;
    if (ix->stagers) ix->stagers->shutdown();
    DeviceGuard g(ix->device);
    (void)hipDeviceSynchronize();
    for (Arr* a : ix->arrays)
        if (a->p && !(a == &ix->raw && ix->raw_borrowed)) (void)hipFree(a->p);
    for (Workspace* w : ix->pool) delete w;
    for (auto& kv : ix->stream_ws) delete kv.second;
    for (auto& sp : ix->stage_prof)
        for (auto& e : sp.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    ix->ev_pool.destroy();
    delete ix;
}

// The header checks of every index type.  brute_force: the brute-force index (no lists; the rotator is FHT-Kac or Matrix).
int validate_header(const rbq_header* h, bool brute_force) {
    if (!h) return fail(RBQ_INVALID_CONFIG, "null header");
    if (h->dim == 0) return fail(RBQ_INVALID_CONFIG, "dimension must be positive");
    if (h->padded_dim < h->dim) return fail(RBQ_INVALID_CONFIG, "padded_dim must be >= dim");
    if (h->metric > 1) return fail(RBQ_INVALID_CONFIG, "unknown metric tag");
    if (h->rotator > (brute_force ? RBQ_ROTATOR_FHT_KAC : RBQ_ROTATOR_NONE)) return fail(RBQ_INVALID_CONFIG, "unknown rotator type tag");
    if (h->ex_bits != 0 && h->ex_bits != 2 && h->ex_bits != 6)
        return fail(RBQ_INVALID_CONFIG, "Unsupported ex_bits: only 0 (1-bit total), 2 (3-bit total), and 6 (7-bit total) are supported");
    if (h->padded_dim % 16 != 0) return fail(RBQ_INVALID_CONFIG, "Dimension must be multiple of 16 for SIMD");
    if (h->padded_dim > 2048)
        return fail(RBQ_INVALID_CONFIG, "padded_dim > 2048 (high-accuracy i32 LUT mode) is not supported");
    if (h->rotator_len != 0 && !h->rotator_blob) return fail(RBQ_INVALID_CONFIG, "null rotator blob");
    if (h->rotator == RBQ_ROTATOR_NONE) {
        if (h->padded_dim != h->dim) return fail(RBQ_INVALID_CONFIG, "rotator NONE requires padded_dim == dim");
        if (h->rotator_len != 0) return fail(RBQ_INVALID_CONFIG, "rotator NONE takes no rotator blob");
    } else if (h->rotator == RBQ_ROTATOR_FHT_KAC) {
        if (h->padded_dim % 64 != 0) return fail(RBQ_INVALID_CONFIG, "FHT rotator requires dimension to be multiple of 64");
        if (h->rotator_len != (uint64_t)4 * h->padded_dim / 8) return fail(RBQ_INVALID_PERSISTENCE, "FHT rotator flip bits length mismatch");
    } else {
        if (h->rotator_len != (uint64_t)h->padded_dim * h->padded_dim * 4) return fail(RBQ_INVALID_PERSISTENCE, "rotator matrix length mismatch");
    }
    if (brute_force) return RBQ_OK;
    if (h->n_lists == 0) return fail(RBQ_INVALID_CONFIG, "nlist must be positive");
    if (h->n_lists > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "too many lists");
    return RBQ_OK;
}

// device list: n_devices ordinals, or the current device
int resolve_devices(int n_devices, const int* devices, std::vector<int>& out) {
    if (n_devices < 1 || n_devices > 16) return fail(RBQ_INVALID_CONFIG, "n_devices must be in 1..16");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    out.clear();
    for (int i = 0; i < n_devices; ++i) {
        int d = 0;
        if (devices) d = devices[i];
        else if (n_devices == 1) HIP_TRY(hipGetDevice(&d));
        else d = i;
        if (d < 0 || d >= count) return fail(RBQ_INVALID_CONFIG, "no such device: " + std::to_string(d));
        out.push_back(d);
    }
    return RBQ_OK;
}

Replica* new_replica(const rbq_header* hdr, int dev) {
    Replica* ix = new Replica();
    static_cast<Geometry&>(*ix) = geometry_of(*hdr);
    ix->device = dev;
    ix->n_lists = hdr->n_lists;
    return ix;
}

// what every construction path shares once list sizes and rotated centroids are on the device: block geometry on
// the host side, centroid-derived arrays, counters, environment switches
int finish_replica(Replica* ix, const std::vector<uint32_t>& ln) {
    const uint32_t nlist = (uint32_t)ix->n_lists, D = ix->D;
    ix->h_list_n = ln;
    ix->nblk_desc_prefix = rbq_host::nblk_desc_prefix(ln);
    const rbq_host::IndexBytes B = index_bytes_of(ix);
    int rc;
    if ((rc = alloc_arr(ix->cnorm2, B.cnorm2))) return rc;
    if ((rc = alloc_arr(ix->cent_hl, B.cent_hl))) return rc;
    HIP_TRY(launch_centroid_arrays((const float*)ix->centroids.p, nlist, D, (float*)ix->cnorm2.p, (uint16_t*)ix->cent_hl.p, 0));
    std::vector<float> cn(nlist);
    HIP_TRY(hipMemcpy(cn.data(), ix->cnorm2.p, (size_t)nlist * 4, hipMemcpyDeviceToHost));
    double mx = 0;
    for (float v : cn) if (std::isfinite(v)) mx = std::max(mx, (double)v);
    ix->cnorm2_max = (float)(mx * 1.000001); // rounded up
    {   // one-product f16 image of the centroids, its residuals and the gate of the route (rank_mfma.hpp header)
        if ((rc = alloc_arr(ix->cent_f16, B.cent_f16))) return rc;
        if ((rc = alloc_arr(ix->cent_f16_resid, B.cent_f16_resid))) return rc;
        HIP_TRY(launch_centroid_f16((const float*)ix->centroids.p, nlist, D, (uint16_t*)ix->cent_f16.p, (float*)ix->cent_f16_resid.p, 0));
        std::vector<float> rs(nlist);
        HIP_TRY(hipMemcpy(rs.data(), ix->cent_f16_resid.p, (size_t)nlist * 4, hipMemcpyDeviceToHost));
        bool finite = true;
        float rmx = 0.0f;
        for (float v : rs) { finite = finite && std::isfinite(v); if (v > rmx) rmx = v; } // (the kernel rounded them up)
        for (float v : cn) finite = finite && std::isfinite(v);
        ix->rc_max = rmx;
        ix->cnorm_max = (float)(std::sqrt(mx * 1.000001) * 1.000001);
        ix->rank_f16_ok = finite && (double)ix->rc_max <= std::ldexp((double)ix->cnorm_max, -11);
    }
    if ((rc = alloc_arr(ix->lsum, B.lsum))) return rc;
    if ((rc = alloc_arr(ix->bsumx, B.bsumx))) return rc;
    HIP_TRY(launch_list_summaries((const uint8_t*)ix->blocks.p, (const uint8_t*)ix->ex.p, (const float*)ix->fadd_ex.p,
                                  (const float*)ix->fres_ex.p, (const float*)ix->centroids.p, (const BlockSummary*)ix->bsum.p,
                                  (const uint32_t*)ix->list_gb0.p, (const uint32_t*)ix->list_n.p, nlist, D, ix->Dc, ix->ex_bits,
                                  (BlockSummaryEx*)ix->bsumx.p, (BlockSummary*)ix->lsum.p, 0));
    if ((rc = alloc_arr(ix->fallbacks, 32))) return rc;   // [0] rank fallbacks, [1] heap restarts, [2] exact-head guard trips, [3] exact-head evaluations,
                                                          // [4..7] tie log: replays, entries replayed, real heap operations, overflowed logs
    HIP_TRY(hipMemset(ix->fallbacks.p, 0, 32));
    if ((rc = alloc_arr(ix->prof, (size_t)kProfStripes * kProfSlots * 8))) return rc;
    HIP_TRY(hipMemset(ix->prof.p, 0, (size_t)kProfStripes * kProfSlots * 8));
    const char* e = std::getenv("RBQ_EXACT_RANK");
    ix->opt.exact_rank = e && e[0] == '1';
    const char* f = std::getenv("RBQ_FORCE_RANK_FALLBACK");
    ix->opt.force_rank_fallback = f && f[0] == '1';
    const char* lz = std::getenv("RBQ_LAZY_SELECT");
    ix->opt.lazy_select = !(lz && lz[0] == '0');
    return RBQ_OK;
}

int Options::set(const char* name, int v) {
    const auto is = [name](const char* n) { return !std::strcmp(name, n); };
    if (is("block_bound")) no_block_bound = v == 0;
    else if (is("exact_rank")) exact_rank = v != 0;
    else if (is("exact_heap")) exact_heap = v != 0;
    else if (is("lazy_select")) lazy_select = v != 0;
    else if (is("rank_tile")) rank_tile = v;
    else if (is("rank_planar")) rank_planar = v != 0;
    else if (is("rank_f16")) rank_f16 = v < 0 ? -1 : (v ? 1 : 0);
    else if (is("latency_path")) latency_path = v;
    else if (is("tie_log")) tie_log = v != 0;
    else if (is("tie_log_cap")) tie_log_cap = v > 0 ? (uint32_t)v : 0u;
    else if (is("stage_mask")) stage_mask = (uint32_t)v & 0xfu;
    else if (is("scan_wave")) scan_wave = v < 0 ? scan_wave_default() : (v > 2 ? 2 : v);
    else if (is("profile_counters")) profile_counters = v != 0;
    else if (is("f32_rank")) f32_rank = v != 0;
    else if (is("wg_prep")) wg_prep = v != 0;
    else if (is("force_rank_fallback")) force_rank_fallback = v != 0;
    else if (is("host_lanes")) host_lanes = v > 0 ? (uint32_t)v : 0u;
    else if (is("host_subbatch")) host_subbatch = v > 0 ? (uint32_t)v : 0u;
    else if (is("host_trace")) host_trace = v != 0;
    else if (is("lazy_fault_inject")) lazy_fault_inject = v != 0;
    else if (is("lazy_audit")) lazy_audit = v != 0;
    else if (is("ub_tap")) ub_tap = v != 0;
    else if (is("save_chunk")) save_chunk = v > 0 ? (uint64_t)v : 0u;
    else if (is("fetch_chunk")) fetch_chunk = v > 0 ? (uint64_t)v : 0u;
    else if (is("mstg_chunk")) mstg_chunk = v > 0 ? (uint64_t)v : 0u;
    else if (is("mstg_search_budget")) mstg_search_budget = v > 0 ? (uint64_t)v : 0u;
    else if (is("slack_term")) slack_term = v;
    else if (is("slack_milli")) { // TEST ONLY: term `slack_term` of block_ub()'s slack times v / 1000 (1000 = the product)
        float* f[6] = {&slack.ge, &slack.eip, &slack.est, &slack.lb, &slack.et, &slack.dist};
        if (slack_term < 0 || slack_term > 5) return fail(RBQ_INVALID_CONFIG, "slack_term is 0..5");
        *f[slack_term] = (float)v * 1e-3f;
    }
    else if (is("head_exact")) head_exact = v != 0;
    else if (is("lazy_filter")) lazy_filter = v != 0;
    else if (is("host_zero_copy")) host_zero_copy = v != 0;
    else if (is("rank_ksplit")) rank_ksplit = v < 0 ? 0 : v;
    else if (is("host_stage_helpers")) host_stage_helpers = v != 0;
    else if (is("rerank_pool")) { // (may be set with or without vectors attached; it acts while the rerank is on and it exceeds top_k)
        if (v > (int)kRerankPoolMax) return fail(RBQ_INVALID_CONFIG, "rerank_pool " + std::to_string(v) + " exceeds the limit of " + std::to_string(kRerankPoolMax));
        rerank_pool = v > 0 ? (uint32_t)v : 0u;
    }
    else if (is("rerank_raw_dtype")) { // what the pointer of the next rbq_index_set_rerank_vectors holds (attached rows keep their own)
        if (v != RBQ_RAW_F32 && v != RBQ_RAW_F16 && v != RBQ_RAW_BF16)
            return fail(RBQ_INVALID_CONFIG, "rerank vectors: unknown dtype " + std::to_string(v) + " (RBQ_RAW_F32, RBQ_RAW_F16 or RBQ_RAW_BF16)");
        rerank_raw_dtype = v;
    }
    else if (is("query_dtype")) { // what every entry point that takes queries reads its pointer as
        if (v != RBQ_RAW_F32 && v != RBQ_RAW_F16 && v != RBQ_RAW_BF16)
            return fail(RBQ_INVALID_CONFIG, "queries: unknown dtype " + std::to_string(v) + " (RBQ_RAW_F32, RBQ_RAW_F16 or RBQ_RAW_BF16)");
        query_dtype = v;
    }
    else if (is("mstg_rerank")) mstg_rerank = v != 0; // (with or without vectors attached; read by rbq_mstg_search_refined_batch* alone)
    else if (is("range_search")) range_search = v != 0;
    else if (is("range_radius_bits")) range_radius_bits = (uint32_t)v; // the 32 bits of an f32 radius: every pattern is a radius
    else if (is("range_exact")) range_exact = v != 0; // (acts while range_search is on: DESIGN.md section 33)
    else if (is("range_exact_radius_bits")) range_exact_radius_bits = (uint32_t)v; // the 32 bits of an f32: every pattern is accepted
    else return fail(RBQ_INVALID_CONFIG, std::string("unknown option ") + name);
    return RBQ_OK;
}
} // namespace rbq_api

namespace rbq_api {
namespace {
void free_index(rbq_index* h) {
    if (!h) return;
    for (auto& w : h->workers) w->shutdown();
    for (Replica* r : h->reps) free_replica(r);
    delete h;
}

// Device-to-device copy between two replicas' devices: peer copy over xGMI when the runtime can (peer access is enabled
// when the devices report it; hipMemcpyPeer itself stages through the host otherwise); if that fails, an explicit bounce
// through a page-locked host buffer, 64 MB at a time.
// RBQ_FORCE_NO_PEER=1 in the environment (read when a handle replicates): every replica copy takes the bounce path, also
// between two replicas on ONE device — the only way the path can run on a one-GPU box (tests/test_gpu_round4.py).
std::atomic<uint64_t> g_bounce_copies{0}; // replica arrays copied through the page-locked bounce buffer (rbq_debug_bounce_copies)
hipError_t copy_cross_device(void* dst, int ddev, const void* src, int sdev, size_t bytes) {
    if (!bytes) return hipSuccess;
    const char* fnp = std::getenv("RBQ_FORCE_NO_PEER");
    const bool no_peer = fnp && fnp[0] == '1';
    hipError_t e = hipSuccess;
    if (!no_peer) {
        if (ddev == sdev) return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice);
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, ddev, sdev) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(sdev, 0); // (current device = ddev)
            if (pe != hipSuccess) (void)hipGetLastError();            // already enabled, or refused: the copy below decides
        } else {
            (void)hipGetLastError();
        }
        e = hipMemcpyPeer(dst, ddev, src, sdev, bytes);
        if (e == hipSuccess) return e;
        (void)hipGetLastError();
    }
    g_bounce_copies.fetch_add(1, std::memory_order_relaxed);
    const size_t CH = (size_t)64 << 20;
    void* bounce = nullptr;
    e = hipHostMalloc(&bounce, std::min(bytes, CH), hipHostMallocPortable);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < bytes && e == hipSuccess; off += CH) {
        const size_t n = std::min(CH, bytes - off);
        e = hipSetDevice(sdev);
        if (e == hipSuccess) e = hipMemcpy(bounce, (const uint8_t*)src + off, n, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipSetDevice(ddev);
        if (e == hipSuccess) e = hipMemcpy((uint8_t*)dst + off, bounce, n, hipMemcpyHostToDevice);
    }
    (void)hipSetDevice(ddev);
    (void)hipHostFree(bounce);
    return e;
}

// A second replica of `src` on device `dev` (may be the same device: exercised by tests on one GPU).
int clone_replica(const Replica* src, int dev, Replica** out) {
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    Replica* ix = new Replica();
    static_cast<Geometry&>(*ix) = *src;
    ix->device = dev;
    ix->n_vectors = src->n_vectors; ix->n_lists = src->n_lists; ix->n_blocks = src->n_blocks;
    ix->cnorm2_max = src->cnorm2_max; ix->cnorm_max = src->cnorm_max; ix->rc_max = src->rc_max; ix->rank_f16_ok = src->rank_f16_ok; ix->h_list_n = src->h_list_n; ix->nblk_desc_prefix = src->nblk_desc_prefix;
    ix->opt = src->opt;
    for (size_t i = 0; i < Replica::kCloned; ++i) {
        const Arr* s = src->arrays[i];
        Arr* d = ix->arrays[i];
        if (!s->p || s == &src->raw) continue;
        hipError_t e = hipMalloc(&d->p, s->bytes ? s->bytes : 16);
        if (e == hipSuccess && s->bytes) e = copy_cross_device(d->p, dev, s->p, src->device, s->bytes);
        if (e != hipSuccess) { free_replica(ix); return fail(RBQ_DEVICE, std::string("replicating the index: ") + hipGetErrorString(e)); }
        d->bytes = s->bytes;
    }
    hipError_t e = hipMemset(ix->fallbacks.p, 0, 32);
    if (e == hipSuccess) e = hipMemset(ix->prof.p, 0, (size_t)kProfStripes * kProfSlots * 8);
    if (e != hipSuccess) { free_replica(ix); return fail(RBQ_DEVICE, hipGetErrorString(e)); }
    *out = ix;
    return RBQ_OK;
}
} // namespace

int wrap_and_replicate(Replica* first, const std::vector<int>& devs, rbq_index** out) {
    rbq_index* h = new rbq_index();
    h->reps.push_back(first);
    for (size_t i = 1; i < devs.size(); ++i) {
        Replica* r = nullptr;
        int rc = clone_replica(first, devs[i], &r);
        if (rc) { free_index(h); return rc; }
        h->reps.push_back(r);
    }
    *out = h;
    return RBQ_OK;
}

namespace {
// ---- create / load: reference layout in, device layout out --------------------------------------------------------
int create_from_sources(const rbq_header* hdr, const std::vector<ListSrc>& lists, int dev, Replica** out) {
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    ReplicaOwner own{new_replica(hdr, dev)};
    Replica* ix = own.ix;
    Scratch cl; // (released before `own`)
    const uint32_t D = ix->D, Dc = ix->Dc, nlist = (uint32_t)ix->n_lists, exbits = ix->ex_bits;
    const size_t ref_stride = (size_t)D * 4 + 384, exb = (size_t)D * exbits / 8;
    std::vector<uint32_t> ln(nlist);
    // the reconstruction factors are kept when every non-empty list brings them
    bool recon = true;
    for (uint32_t c = 0; c < nlist; ++c)
        if (lists[c].n && (!lists[c].delta || !lists[c].vl)) recon = false;
    for (uint32_t c = 0; c < nlist; ++c) {
        if (lists[c].n > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "list too large"); // (create_impl and rbq1_parse have refused it)
        ln[c] = (uint32_t)lists[c].n;
    }
    rbq_host::ListLayout lay;
    std::string detail;
    if (!rbq_host::list_layout(ln.data(), nlist, &lay, &detail)) return fail(RBQ_INVALID_CONFIG, detail);
    const uint64_t nblocks = lay.blocks;
    int rc;
    if ((rc = upload_arr(ix->rot_blob, hdr->rotator_blob, hdr->rotator_len))) return rc;
    // (the pad of `ex` is zeroed here, synchronously, not behind the chunk loop on its stream: the chunk kernels write slot bytes
    // only, never those 256, and the device is idle before the replica is handed on)
    if ((rc = alloc_index_arrays(ix, ln, lay.gb0, nblocks, lay.vectors, recon, /*rnorm=*/false))) return rc;
    const rbq_host::IndexBytes B = index_bytes_of(ix);
    const size_t dev_stride = B.block_stride, exd = B.ex_slot;
    {
        std::vector<float> cent((size_t)nlist * D);
        for (uint32_t c = 0; c < nlist; ++c) std::memcpy(&cent[(size_t)c * D], lists[c].centroid, (size_t)D * 4);
        if ((rc = upload_arr(ix->centroids, cent.data(), cent.size() * 4))) return rc;
    }

    // Chunks of whole blocks (a long list may span several), staged through two pinned buffers: the host fills
    // one while the GPU converts the other.  Staging layout (16-byte aligned sections):
    //   recs [nb][ref_stride] | ex [nv][exb] | ids [nv] u64 | fadd [nv] f32 | fres [nv] f32 | delta [nv] f32 | vl [nv] f32 |
    //   dense0 [nb] u64 | nvb [nb] u32
    const size_t per_block = ref_stride + 32 * (exb + 24) + 12 + 64;
    uint64_t chunk_blocks = std::max<uint64_t>(1, ((size_t)64 << 20) / per_block);
    chunk_blocks = std::min<uint64_t>(chunk_blocks, std::max<uint64_t>(nblocks, 1));
    const size_t cap = align_up(chunk_blocks * ref_stride, 16) + align_up(chunk_blocks * 32 * exb, 16) + chunk_blocks * 32 * 24 +
                       chunk_blocks * 12 + 256;
    uint8_t* pin[2] = {nullptr, nullptr};
    uint8_t* dst[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(cl.make_stream());
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(cl.alloc_pinned(&pin[i], cap));
        HIP_TRY(cl.alloc(&dst[i], cap));
        HIP_TRY(cl.event(&ev[i]));
    }
    uint32_t c = 0;      // list cursor
    uint64_t lb = 0;     // next block inside list c
    uint64_t b0 = 0;     // first global block of the chunk
    int turn = 0;
    while (b0 < nblocks) {
        const uint64_t nb = std::min<uint64_t>(chunk_blocks, nblocks - b0);
        const int i = turn & 1;
        if (turn >= 2) HIP_TRY(hipEventSynchronize(ev[i]));
        uint8_t* base = pin[i];
        const size_t o_recs = 0, o_ex = align_up(nb * ref_stride, 16);
        // the number of vectors of the chunk is known only after the walk: lay the dense arrays out for the maximum
        const size_t o_ids = o_ex + align_up(nb * 32 * exb, 16), o_fadd = o_ids + nb * 32 * 8, o_fres = o_fadd + nb * 32 * 4,
                     o_dl = o_fres + nb * 32 * 4, o_vl = o_dl + nb * 32 * 4, o_d0 = o_vl + nb * 32 * 4, o_nv = o_d0 + nb * 8,
                     total = o_nv + nb * 4;
        uint64_t* dense0 = reinterpret_cast<uint64_t*>(base + o_d0);
        uint32_t* nvb = reinterpret_cast<uint32_t*>(base + o_nv);
        uint64_t filled = 0, dense = 0;
        while (filled < nb) {
            while (c < nlist && lb >= rbq_host::blocks_of(ln[c])) { ++c; lb = 0; }
            const ListSrc& L = lists[c];
            const uint64_t lnb = rbq_host::blocks_of(ln[c]), take = std::min<uint64_t>(lnb - lb, nb - filled);
            const uint64_t v0 = lb * 32, v1 = std::min<uint64_t>(L.n, (lb + take) * 32), nv = v1 - v0;
            std::memcpy(base + o_recs + filled * ref_stride, L.batch_data + lb * ref_stride, take * ref_stride);
            if (nv) std::memcpy(base + o_ids + dense * 8, L.ids + v0 * 8, nv * 8);
            if (exbits && nv) {
                if (L.ex_stride == exb) std::memcpy(base + o_ex + dense * exb, L.ex + v0 * exb, nv * exb);
                else for (uint64_t v = 0; v < nv; ++v) std::memcpy(base + o_ex + (dense + v) * exb, L.ex + (v0 + v) * L.ex_stride, exb);
                std::memcpy(base + o_fadd + dense * 4, L.fadd + v0 * 4, nv * 4);
                std::memcpy(base + o_fres + dense * 4, L.fres + v0 * 4, nv * 4);
            }
            if (recon && nv) {
                std::memcpy(base + o_dl + dense * 4, L.delta + v0 * 4, nv * 4);
                std::memcpy(base + o_vl + dense * 4, L.vl + v0 * 4, nv * 4);
            }
            for (uint64_t b = 0; b < take; ++b) {
                dense0[filled + b] = dense + b * 32;
                nvb[filled + b] = (uint32_t)std::min<uint64_t>(32, L.n - (lb + b) * 32);
            }
            filled += take; dense += nv; lb += take;
        }
        uint8_t* d = dst[i];
        HIP_TRY(hipMemcpyAsync(d, base, total, hipMemcpyHostToDevice, cl.stream));
        const uint64_t* d_d0 = reinterpret_cast<const uint64_t*>(d + o_d0);
        const uint32_t* d_nv = reinterpret_cast<const uint32_t*>(d + o_nv);
        uint8_t* oblocks = (uint8_t*)ix->blocks.p + b0 * dev_stride;
        HIP_TRY(launch_relayout_blocks(d + o_recs, (uint32_t)nb, D, Dc, oblocks, cl.stream));
        HIP_TRY(launch_block_summary(oblocks, d_nv, (uint32_t)nb, Dc, (BlockSummary*)ix->bsum.p + b0, cl.stream));
        HIP_TRY(launch_spread_u64(reinterpret_cast<const uint64_t*>(d + o_ids), d_d0, d_nv, (uint32_t)nb, ~0ull,
                                  (uint64_t*)ix->ids.p + b0 * 32, cl.stream));
        if (exbits) {
            HIP_TRY(launch_relayout_ex(d + o_ex, d_d0, d_nv, (uint32_t)nb, D, exbits, (uint8_t*)ix->ex.p + b0 * 32 * exd, cl.stream));
            HIP_TRY(launch_spread_f32(reinterpret_cast<const float*>(d + o_fadd), d_d0, d_nv, (uint32_t)nb, 0.0f,
                                      (float*)ix->fadd_ex.p + b0 * 32, cl.stream));
            HIP_TRY(launch_spread_f32(reinterpret_cast<const float*>(d + o_fres), d_d0, d_nv, (uint32_t)nb, 0.0f,
                                      (float*)ix->fres_ex.p + b0 * 32, cl.stream));
        }
        if (recon) {
            HIP_TRY(launch_spread_f32(reinterpret_cast<const float*>(d + o_dl), d_d0, d_nv, (uint32_t)nb, 0.0f,
                                      (float*)ix->delta.p + b0 * 32, cl.stream));
            HIP_TRY(launch_spread_f32(reinterpret_cast<const float*>(d + o_vl), d_d0, d_nv, (uint32_t)nb, 0.0f,
                                      (float*)ix->vl.p + b0 * 32, cl.stream));
        }
        HIP_TRY(hipEventRecord(ev[i], cl.stream));
        b0 += nb;
        ++turn;
    }
    HIP_TRY(hipStreamSynchronize(cl.stream));
    if ((rc = finish_replica(ix, ln))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = own.release();
    return RBQ_OK;
}

// delta / vl: null (rbq_index_create: no reconstruction factors) or n_lists pointers to n f32 each
int create_impl(const rbq_header* hdr, const rbq_list_view* lists, const float* const* delta, const float* const* vl, int n_devices,
                const int* devices, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    int rc = validate_header(hdr);
    if (rc) return rc;
    if (!lists) return fail(RBQ_INVALID_CONFIG, "null lists");
    if (!delta != !vl) return fail(RBQ_INVALID_CONFIG, "delta and vl are given together");
    std::vector<int> devs;
    if ((rc = resolve_devices(n_devices, devices, devs))) return rc;
    const size_t ref_stride = (size_t)hdr->padded_dim * 4 + 384, exb = (size_t)hdr->padded_dim * hdr->ex_bits / 8;
    std::vector<ListSrc> src(hdr->n_lists);
    for (uint64_t c = 0; c < hdr->n_lists; ++c) {
        const rbq_list_view& L = lists[c];
        if (L.n > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "list too large");
        const uint64_t nb = rbq_host::blocks_of(L.n);
        if (L.batch_len != nb * ref_stride)
            return fail(RBQ_INVALID_PERSISTENCE, "batch_data length mismatch - possible corruption or version incompatibility");
        if (L.n && (!L.centroid || !L.ids || !L.batch_data || (hdr->ex_bits && (!L.ex_codes || !L.f_add_ex || !L.f_rescale_ex))))
            return fail(RBQ_INVALID_CONFIG, "null list array");
        if (!L.centroid) return fail(RBQ_INVALID_CONFIG, "null centroid");
        ListSrc& S = src[c];
        S.centroid = (const uint8_t*)L.centroid; S.n = L.n; S.ids = (const uint8_t*)L.ids; S.batch_data = L.batch_data;
        S.ex = L.ex_codes; S.ex_stride = exb; S.fadd = (const uint8_t*)L.f_add_ex; S.fres = (const uint8_t*)L.f_rescale_ex;
        if (delta) {
            if (L.n && (!delta[c] || !vl[c])) return fail(RBQ_INVALID_CONFIG, "null delta / vl array");
            S.delta = (const uint8_t*)delta[c]; S.vl = (const uint8_t*)vl[c];
        }
    }
    Replica* first = nullptr;
    if ((rc = create_from_sources(hdr, src, devs[0], &first))) return rc;
    return wrap_and_replicate(first, devs, out);
}

int load_rbq1_impl(const void* bytes, size_t len, int n_devices, const int* devices, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    rbq_header h;
    std::vector<ListSrc> lists; // byte ranges of the stream: nothing is copied on the host but the chunk staging
    std::string detail;
    int rc = rbq_host::rbq1_parse(bytes, len, &h, &lists, &detail); // load_from_reader's validation, CRC included
    if (rc) return fail(rc, detail);
    rc = validate_header(&h); // what this build cannot serve (ex_bits outside {0,2,6}, padded_dim > 2048 ...)
    if (rc) return rc;
    std::vector<int> devs;
    if ((rc = resolve_devices(n_devices, devices, devs))) return rc;
    Replica* first = nullptr;
    if ((rc = create_from_sources(&h, lists, devs[0], &first))) return rc;
    return wrap_and_replicate(first, devs, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
// (minor 1: rbq_debug_tie_log_stats; options latency_path, tie_log.  minor 2: rbq_index_set_numeric_variant / rbq_index_numeric_variant)
uint32_t rbq_abi_version(void) { return (2u << 16) | 2u; }

const char* rbq_strerror(int code) {
    switch (code) {
        case RBQ_OK: return "ok";
        case RBQ_DIMENSION_MISMATCH: return "dimension mismatch";
        case RBQ_INVALID_CONFIG: return "invalid configuration";
        case RBQ_EMPTY_INDEX: return "index is empty";
        case RBQ_IO: return "io error";
        case RBQ_INVALID_PERSISTENCE: return "invalid persisted index";
        case RBQ_DEVICE: return "device error";
        default: return "unknown error";
    }
}

int rbq_last_error_detail(char* buf, size_t n) {
    if (buf && n) {
        size_t c = std::min(n - 1, g_err.size());
        std::memcpy(buf, g_err.data(), c);
        buf[c] = 0;
    }
    return (int)g_err.size();
}

int rbq_index_create(const rbq_header* hdr, const rbq_list_view* lists, int n_devices, const int* devices, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return create_impl(hdr, lists, nullptr, nullptr, n_devices, devices, out);
    RBQ_GUARD_END
}

void rbq_index_destroy(rbq_index* h) { try { free_index(h); } catch (...) {} }

uint64_t rbq_index_len(const rbq_index* h) { return h && !h->reps.empty() ? h->reps[0]->n_vectors : 0; }
uint64_t rbq_index_cluster_count(const rbq_index* h) { return h && !h->reps.empty() ? h->reps[0]->n_lists : 0; }
uint32_t rbq_index_dim(const rbq_index* h) { return h && !h->reps.empty() ? h->reps[0]->dim : 0; }
uint32_t rbq_index_padded_dim(const rbq_index* h) { return h && !h->reps.empty() ? h->reps[0]->D : 0; }
uint32_t rbq_index_device_count(const rbq_index* h) { return h ? (uint32_t)h->reps.size() : 0; }


int rbq_index_load_rbq1(const void* bytes, size_t len, int n_devices, const int* devices, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return load_rbq1_impl(bytes, len, n_devices, devices, out);
    RBQ_GUARD_END
}


int rbq_index_create_with_recon(const rbq_header* hdr, const rbq_list_view* lists, const float* const* delta, const float* const* vl,
                                int n_devices, const int* devices, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!delta || !vl) return fail(RBQ_INVALID_CONFIG, "null delta / vl table");
    return create_impl(hdr, lists, delta, vl, n_devices, devices, out);
    RBQ_GUARD_END
}


// ---- optional full-precision rerank (NOT in the reference: its index stores no raw vectors, src/ivf.rs:207-242) ----
// The rows are dim elements of the handle's option "rerank_raw_dtype" (RBQ_RAW_*, f32 unless set; Options::set admits no other
// value): a 16-bit element is widened exactly where a kernel loads it, nothing is converted here.
int rbq_index_set_rerank_vectors(rbq_index* h, const float* vectors_f32, uint64_t n) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!h || h->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    const void* vectors = vectors_f32;
    const int dtype = h->reps[0]->opt.rerank_raw_dtype;
    const size_t esize = raw_elem_bytes(dtype);
    // all replicas or none: the new copies are made first; only when every one of them exists are the old ones released
    // and the new ones attached (a failure half-way leaves every replica exactly as it was)
    const size_t R = h->reps.size();
    std::vector<Arr> fresh(R);
    std::vector<char> borrowed(R, 0);
    const bool attach = vectors && n;
    if (attach) {
        hipPointerAttribute_t a;
        const bool on_dev = hipPointerGetAttributes(&a, vectors) == hipSuccess && a.type == hipMemoryTypeDevice;
        if (!on_dev) (void)hipGetLastError();
        if (on_dev && esize == 2 && (reinterpret_cast<uintptr_t>(vectors) & 1u))
            return fail(RBQ_INVALID_CONFIG, "rerank vectors: a device pointer to 16-bit rows must be 2-byte aligned");
        int rc = RBQ_OK;
        for (size_t r = 0; r < R && rc == RBQ_OK; ++r) {
            Replica* ix = h->reps[r];
            DeviceGuard g(ix->device);
            if (!g.ok) { rc = fail(RBQ_DEVICE, "hipSetDevice failed"); break; }
            const size_t bytes = (size_t)n * ix->dim * esize;
            if (on_dev && a.device == ix->device) { // borrowed: stays owned by the caller, must outlive the index
                fresh[r].p = const_cast<void*>(vectors); fresh[r].bytes = bytes; borrowed[r] = 1;
                continue;
            }
            rc = alloc_arr(fresh[r], bytes);
            if (rc == RBQ_OK) {
                const hipError_t e = on_dev ? copy_cross_device(fresh[r].p, ix->device, vectors, a.device, bytes)
                                            : hipMemcpy(fresh[r].p, vectors, bytes, hipMemcpyHostToDevice);
                if (e != hipSuccess) rc = fail(RBQ_DEVICE, std::string("attaching the rerank vectors: ") + hipGetErrorString(e));
            }
        }
        if (rc != RBQ_OK) {
            const std::string keep = g_err;
            for (size_t r = 0; r < R; ++r)
                if (fresh[r].p && !borrowed[r]) { DeviceGuard g(h->reps[r]->device); (void)hipFree(fresh[r].p); }
            return fail(rc, keep);
        }
    }
    for (size_t r = 0; r < R; ++r) {
        Replica* ix = h->reps[r];
        DeviceGuard g(ix->device);
        if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
        HIP_TRY(hipDeviceSynchronize());
        if (ix->raw.p && !ix->raw_borrowed) (void)hipFree(ix->raw.p);
        ix->raw = Arr(); ix->n_raw = 0; ix->rerank = false; ix->raw_borrowed = false; ix->raw_dtype = RBQ_RAW_F32;
        if (!attach) continue; // detach
        ix->raw = fresh[r]; ix->raw_borrowed = borrowed[r] != 0; ix->raw_dtype = dtype;
        ix->n_raw = n; ix->rerank = true;
    }
    return RBQ_OK;
    RBQ_GUARD_END
}

// ---- pinned host memory for callers that want zero-copy DMA of queries and results ---------------------
void* rbq_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void rbq_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- profiling taps ---------------------------------------------------------------------------------
void rbq_profile_begin(rbq_index* h) {
    if (!h) return;
    for (Replica* ix : h->reps) {
        DeviceGuard g(ix->device);
        std::lock_guard<std::mutex> lk(ix->mu);
        for (auto& sp : ix->stage_prof) {
            for (auto& e : sp.ev) ix->ev_pool.give(e);
            sp.ev.clear(); sp.ms = 0; sp.launches = 0; sp.samples.clear();
        }
        for (auto& c : ix->prof_counters) c = 0;
        (void)hipMemset(ix->prof.p, 0, (size_t)kProfStripes * kProfSlots * 8);
        ix->profiling = true;
    }
}
void rbq_profile_end(rbq_index* h) {
    if (!h) return;
    for (Replica* ix : h->reps) {
        DeviceGuard g(ix->device);
        (void)hipDeviceSynchronize();
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->profiling = false;
        std::vector<unsigned long long> c((size_t)kProfStripes * kProfSlots, 0ull);
        (void)hipMemcpy(c.data(), ix->prof.p, c.size() * 8, hipMemcpyDeviceToHost);
        for (int i = 0; i < kProfSlots; ++i) {
            ix->prof_counters[i] = 0;
            for (uint32_t st = 0; st < kProfStripes; ++st) ix->prof_counters[i] += c[(size_t)st * kProfSlots + i];
        }
        for (auto& sp : ix->stage_prof) {
            for (auto& e : sp.ev) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { sp.ms += ms; sp.launches++; sp.samples.push_back(ms); }
                ix->ev_pool.give(e);
            }
            sp.ev.clear();
        }
    }
}
// index of a profiled stage in Replica::stage_prof, or -1 (no handle, no replica, unknown name)
static int profile_stage_index(const rbq_index* h, const char* stage) {
    if (!h || h->reps.empty() || !stage) return -1;
    static const char* const names[4] = {"prep", "rank", "select", "scan"};
    for (int s = 0; s < 4; ++s) if (!std::strcmp(stage, names[s])) return s;
    return -1;
}
double rbq_profile_stage_ms(const rbq_index* h, const char* stage, uint64_t* launches) {
    const int s = profile_stage_index(h, stage);
    if (s < 0) return -1;
    double ms = 0; uint64_t n = 0;
    for (const Replica* ix : h->reps) { ms += ix->stage_prof[s].ms; n += ix->stage_prof[s].launches; }
    if (launches) *launches = n;
    return n ? ms / (double)n : 0.0;
}
uint64_t rbq_profile_stage_samples(const rbq_index* h, const char* stage, float* out, uint64_t cap) {
    const int s = profile_stage_index(h, stage);
    if (s < 0) return 0;
    uint64_t n = 0;
    for (const Replica* ix : h->reps)
        for (float v : ix->stage_prof[s].samples) { if (out && n < cap) out[n] = v; ++n; }
    return n;
}
uint64_t rbq_profile_scan_bytes(const rbq_index* h) {
    if (!h || h->reps.empty()) return 0;
    uint64_t v = 0;
    for (const Replica* ix : h->reps) v += ix->prof_counters[kProfVectorsProbed];
    return v * (uint64_t)(h->reps[0]->D / 8 + 12); // sum_q sum_{c in probe(q)} n_c * (D/8 + 12)
}
int rbq_profile_counters(const rbq_index* h, uint64_t* out, uint32_t n) {
    if (!h || h->reps.empty() || !out) return RBQ_INVALID_CONFIG;
    for (uint32_t i = 0; i < n; ++i) {
        out[i] = 0;
        if (i < (uint32_t)kProfSlots) for (const Replica* ix : h->reps) out[i] += ix->prof_counters[i];
    }
    return RBQ_OK;
}
void rbq_profile_select_stages(rbq_index* h, uint32_t mask) { if (h) for (Replica* ix : h->reps) ix->prof_mask = mask & 0xfu; }
void rbq_profile_set_sampling(rbq_index* h, uint32_t every) { if (h) for (Replica* ix : h->reps) ix->prof_every = every ? every : 1u; }

int rbq_index_set_numeric_variant(rbq_index* h, int variant) {
    g_err.clear();
    if (!h || h->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    if (variant != RBQ_NUMERIC_NATIVE_AVX512 && variant != RBQ_NUMERIC_NATIVE_AVX2 && variant != RBQ_NUMERIC_PORTABLE)
        return fail(RBQ_INVALID_CONFIG, "numeric variant " + std::to_string(variant) +
                                            " is not one of 0 (native_avx512), 1 (native_avx2), 2 (portable)");
    static_assert(RBQ_NUMERIC_NATIVE_AVX512 == kVarAvx512 && RBQ_NUMERIC_NATIVE_AVX2 == kVarAvx2 && RBQ_NUMERIC_PORTABLE == kVarPortable,
                  "the ABI values are the kernels' variant numbers");
    for (Replica* ix : h->reps) ix->opt.numeric_variant = (uint32_t)variant;
    return RBQ_OK;
}
int rbq_index_numeric_variant(const rbq_index* h) {
    if (!h || h->reps.empty()) return -1;
    return (int)h->reps[0]->opt.numeric_variant;
}

int rbq_debug_set_option(rbq_index* h, const char* name, int value) {
    if (!h || h->reps.empty() || !name) return RBQ_INVALID_CONFIG;
    if (!std::strcmp(name, "numeric_variant")) return rbq_index_set_numeric_variant(h, value);
    if (!std::strcmp(name, "debug_replica")) {
        if (value < 0 || (size_t)value >= h->reps.size()) return fail(RBQ_INVALID_CONFIG, "no such replica");
        h->debug_replica = value;
        return RBQ_OK;
    }
    for (Replica* ix : h->reps) {
        int rc;
        if (!std::strcmp(name, "rerank")) {
            if (value && !ix->raw.p) return fail(RBQ_INVALID_CONFIG, "no raw vectors attached (rbq_index_set_rerank_vectors)");
            ix->rerank = value != 0;
        } else if ((rc = ix->opt.set(name, value))) {
            return rc;
        }
    }
    return RBQ_OK;
}
static uint64_t read_counter(const rbq_index* h, int slot) {
    if (!h) return 0;
    uint64_t tot = 0;
    for (const Replica* ix : h->reps) {
        unsigned int v = 0;
        DeviceGuard g(ix->device);
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(&v, (const unsigned int*)ix->fallbacks.p + slot, 4, hipMemcpyDeviceToHost);
        tot += v;
    }
    return tot;
}
uint64_t rbq_debug_rank_fallbacks(const rbq_index* h) { return read_counter(h, 0); }
void rbq_debug_tie_log_stats(const rbq_index* h, uint64_t* out4) { if (out4) for (int i = 0; i < 4; ++i) out4[i] = read_counter(h, 4 + i); }
uint64_t rbq_debug_head_exact_guard_trips(const rbq_index* h) { return read_counter(h, 2); }
uint64_t rbq_debug_head_exact_evaluations(const rbq_index* h) { return read_counter(h, 3); }


uint64_t rbq_debug_bounce_copies(void) { return g_bounce_copies.load(std::memory_order_relaxed); }
uint64_t rbq_debug_heap_restarts(const rbq_index* h) { return read_counter(h, 1); }


namespace {
// 0 / 1 when `name` is the hi / lo plane's name, else -1
int hl_plane_of(const char* name, const char* hi, const char* lo) { return !std::strcmp(name, hi) ? 0 : (!std::strcmp(name, lo) ? 1 : -1); }
// host mirror of the interleaved split-bf16 image (hl_layout.hpp): plane `plane` of `rows` rows at d_hl, [rows][D] u16, to dst
int copy_hl_plane(const void* d_hl, uint64_t rows, uint32_t D, int plane, void* dst) {
    std::vector<uint16_t> hl((size_t)rows * 2 * D);
    HIP_TRY(hipMemcpy(hl.data(), d_hl, hl.size() * 2, hipMemcpyDeviceToHost));
    uint16_t* out = (uint16_t*)dst;
    for (uint64_t r = 0; r < rows; ++r)
        for (uint32_t i = 0; i < D; ++i) out[r * D + i] = hl[r * 2 * D + hl_offset(i, (uint32_t)plane, D)];
    return RBQ_OK;
}
} // namespace

/* Diagnostic: copy an intermediate buffer of the workspace bound to `hip_stream` (after the caller synchronised). */
int rbq_debug_copy_workspace(rbq_index* h, void* hip_stream, const char* name, void* dst, uint64_t bytes) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!h || h->reps.empty() || !name || !dst) return RBQ_INVALID_CONFIG;
    Replica* ix = h->reps[h->debug_replica];
    Workspace* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        auto it = ix->stream_ws.find((hipStream_t)hip_stream);
        if (it != ix->stream_ws.end()) w = it->second;
    }
    if (!w) return fail(RBQ_INVALID_CONFIG, "no workspace for this stream");
    static const std::pair<const char*, DevBuf Workspace::*> kBufs[] = {
        {"rot", &Workspace::rot}, {"lut", &Workspace::lut}, {"consts", &Workspace::consts}, {"scores", &Workspace::scores},
        {"probe", &Workspace::probe}, {"nstream", &Workspace::nstream}, {"wl", &Workspace::wl}, {"nvec", &Workspace::nvec},
        {"dead_skipped", &Workspace::dead_skipped}, {"audit_dead", &Workspace::audit_dead}, {"head_ub", &Workspace::head_ub},
        {"rot_hl", &Workspace::rot_hl}, {"rot_f16", &Workspace::rot_f16}, {"rank_resid", &Workspace::rank_resid}};
    DeviceGuard g(ix->device);
    if (const int plane = hl_plane_of(name, "rot_hi", "rot_lo"); plane >= 0) { // logical view: whole rows of [D] u16
        const size_t row = (size_t)ix->D * 2;
        if (!w->rot_hl.p || bytes % row || bytes * 2 > w->rot_hl.cap) return fail(RBQ_INVALID_CONFIG, "unknown buffer or size");
        return copy_hl_plane(w->rot_hl.p, bytes / row, ix->D, plane, dst);
    }
    DevBuf* b = nullptr;
    for (const auto& kb : kBufs) if (!std::strcmp(name, kb.first)) b = &(w->*kb.second);
    if (!b || !b->p || bytes > b->cap) return fail(RBQ_INVALID_CONFIG, "unknown buffer or size");
    HIP_TRY(hipMemcpy(dst, b->p, bytes, hipMemcpyDeviceToHost));
    return RBQ_OK;
    RBQ_GUARD_END
}

/* Diagnostic: copy one of the index's device arrays to the host. */
int rbq_debug_copy_index(rbq_index* h, const char* name, void* dst, uint64_t bytes) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!h || h->reps.empty() || !name || !dst) return RBQ_INVALID_CONFIG;
    Replica* ix = h->reps[h->debug_replica];
    using rbq_host::IndexBytes;
    const IndexBytes B = index_bytes_of(ix); // (every replica has the first one's geometry)
    static const struct { const char* name; Arr Replica::*arr; size_t IndexBytes::*bytes; } kArrays[] = {
        {"blocks", &Replica::blocks, &IndexBytes::blocks}, {"ids", &Replica::ids, &IndexBytes::ids}, {"ex", &Replica::ex, &IndexBytes::ex},
        {"fadd_ex", &Replica::fadd_ex, &IndexBytes::fadd_ex}, {"fres_ex", &Replica::fres_ex, &IndexBytes::fres_ex},
        {"bsum", &Replica::bsum, &IndexBytes::bsum}, {"lsum", &Replica::lsum, &IndexBytes::lsum}, {"bsumx", &Replica::bsumx, &IndexBytes::bsumx},
        {"centroids", &Replica::centroids, &IndexBytes::centroids}, {"list_gb0", &Replica::list_gb0, &IndexBytes::list_gb0},
        {"list_n", &Replica::list_n, &IndexBytes::list_n}, {"cent_hl", &Replica::cent_hl, &IndexBytes::cent_hl},
        {"cent_f16", &Replica::cent_f16, &IndexBytes::cent_f16}, {"cent_f16_resid", &Replica::cent_f16_resid, &IndexBytes::cent_f16_resid},
        {"cnorm2", &Replica::cnorm2, &IndexBytes::cnorm2}};
    const void* p = nullptr;
    size_t have = 0;
    if (!std::strcmp(name, "rerank_raw_dtype")) { // (not an array: RBQ_RAW_* of the attached rerank rows as one int32, -1 with none attached)
        if (bytes != 4) return fail(RBQ_INVALID_CONFIG, "rerank_raw_dtype is one int32");
        const int32_t v = h->reps[0]->raw.p ? h->reps[0]->raw_dtype : -1;
        std::memcpy(dst, &v, 4);
        return RBQ_OK;
    }
    if (!std::strcmp(name, "mstg_rerank")) { // (not an array: the option "mstg_rerank" as the handle holds it, one int32)
        if (bytes != 4) return fail(RBQ_INVALID_CONFIG, "mstg_rerank is one int32");
        const int32_t v = h->reps[0]->opt.mstg_rerank ? 1 : 0;
        std::memcpy(dst, &v, 4);
        return RBQ_OK;
    }
    if (!std::strcmp(name, "query_dtype")) { // (not an array: the option "query_dtype" as the handle holds it, one int32)
        if (bytes != 4) return fail(RBQ_INVALID_CONFIG, "query_dtype is one int32");
        const int32_t v = h->reps[0]->opt.query_dtype;
        std::memcpy(dst, &v, 4);
        return RBQ_OK;
    }
    if (!std::strcmp(name, "metric")) { // (not an array: the handle's metric as one int32, 0 = L2, 1 = inner product)
        if (bytes != 4) return fail(RBQ_INVALID_CONFIG, "metric is one int32");
        const int32_t v = (int32_t)h->reps[0]->metric;
        std::memcpy(dst, &v, 4);
        return RBQ_OK;
    }
    if (const int plane = hl_plane_of(name, "cent_hi", "cent_lo"); plane >= 0) { // logical view of "cent_hl"
        if (!ix->cent_hl.p || bytes != B.cent_hl / 2)
            return fail(RBQ_INVALID_CONFIG, "unknown array or size (have " + std::to_string(B.cent_hl / 2) + " bytes)");
        DeviceGuard g(ix->device);
        return copy_hl_plane(ix->cent_hl.p, ix->n_lists, ix->D, plane, dst);
    }
    for (const auto& a : kArrays)
        if (!std::strcmp(name, a.name)) { p = (ix->*a.arr).p; have = B.*a.bytes; }
    if (!std::strcmp(name, "delta") || !std::strcmp(name, "vl")) { // (first replica only)
        ix = h->reps[0];
        p = name[0] == 'd' ? ix->delta.p : ix->vl.p; have = ix->has_recon ? B.delta : 0;
    }
    else if (!std::strcmp(name, "rnorm")) { // (first replica only; MSTG handles)
        ix = h->reps[0];
        p = ix->rnorm.p; have = ix->has_rnorm ? B.rnorm : 0;
    }
    if (!p || bytes != have) return fail(RBQ_INVALID_CONFIG, "unknown array or size (have " + std::to_string(have) + " bytes)");
    DeviceGuard g(ix->device);
    HIP_TRY(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return RBQ_OK;
    RBQ_GUARD_END
}
} // extern "C"
