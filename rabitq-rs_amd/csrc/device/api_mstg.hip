// api_mstg.hip — MSTG build (include/rbq_mstg.h): hierarchical balanced clustering (k_hcluster.hip), closure assignment on the
// device (k_mstg.hip) and the device encoder of api_build.hip fed the expanded (vector, list) pairs.
#include "api.hpp"
#include "rbq_mstg.h"
#include "../host/rbq_hcluster.hpp"

using namespace rbq_api;

struct rbq_hclustered { rbq_host::HcResult r; };

static_assert(RBQ_MSTG_MAX_REPLICAS == kMstgMaxReplicas, "rbq_mstg.h and launch.hpp disagree");

namespace rbq_api {
namespace {
std::atomic<uint64_t> g_closure_fallbacks{0};

// what ClosureAssigner::assign would panic on, and what this build does not serve; no HIP call
int check_closure_args(const float* centroids, uint64_t n_lists, uint32_t dim, const float* data, uint64_t n, float epsilon,
                       uint32_t max_replicas) {
    if (!centroids || !data) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (n == 0) return fail(RBQ_INVALID_CONFIG, "no vectors");
    if (n > 0xfffffff0ull) return fail(RBQ_INVALID_CONFIG, "too many vectors for 32-bit slots");
    if (n_lists == 0) return fail(RBQ_INVALID_CONFIG, "nlist must be positive");
    if (n_lists >= 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "too many lists");
    if (dim == 0) return fail(RBQ_INVALID_CONFIG, "dimension must be positive");
    if (max_replicas == 0) return fail(RBQ_INVALID_CONFIG, "max_replicas must be positive");
    if (max_replicas > kMstgMaxReplicas) return fail(RBQ_INVALID_CONFIG, "max_replicas above 64 is not supported");
    if (!(epsilon >= 0.0f) || !std::isfinite(epsilon)) return fail(RBQ_INVALID_CONFIG, "closure epsilon must be finite and not negative");
    return RBQ_OK;
}

} // namespace

int run_closure(ClosureArgs& a, int dev, bool count) { // (api.hpp: rbq_mstg_append runs it too)
    a.cent_on_device = is_device_pointer(a.centroids);
    a.data_on_device = is_device_pointer(a.data);
    a.out_on_device = a.out_lists && is_device_pointer(a.out_lists);
    if (a.out_lists && a.out_on_device != is_device_pointer(a.out_counts))
        return fail(RBQ_INVALID_CONFIG, "out_lists and out_counts must both be host or both be device memory");
    uint64_t fb = 0;
    a.fallbacks = &fb;
    std::string detail;
    const int rc = closure_device(a, dev, detail);
    if (rc) return fail(rc, detail);
    if (count) g_closure_fallbacks.fetch_add(fb, std::memory_order_relaxed);
    return RBQ_OK;
}

namespace {

int build_impl(const rbq_header* hdr, const float* centroids, const float* data, uint64_t n, float epsilon, uint32_t max_replicas,
               int rescale, float t_const, uint64_t max_chunk_rows, int device, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    int rc = validate_header(hdr);
    if (rc) return rc;
    if (hdr->rotator != RBQ_ROTATOR_NONE) return fail(RBQ_INVALID_CONFIG, "MSTG posting lists take rotator RBQ_ROTATOR_NONE");
    if ((rc = check_closure_args(centroids, hdr->n_lists, hdr->dim, data, n, epsilon, max_replicas))) return rc;
    const int opt = rescale_mode(rescale, hdr);
    if (opt < 0) return RBQ_INVALID_CONFIG;
    if (!opt && hdr->ex_bits > 0 && !(t_const > 0.0f)) return fail(RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)");
    std::vector<int> devs;
    if ((rc = resolve_devices(1, device < 0 ? nullptr : &device, devs))) return rc;
    const int dev = devs[0];
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    const uint32_t dim = hdr->dim, M = max_replicas;
    const uint64_t k = hdr->n_lists;
    Scratch t;
    // the encoder gathers rows by list: host data is uploaded whole; it takes the centroids from host memory
    const float* d_data = data;
    if (!is_device_pointer(data)) {
        float* p = nullptr;
        HIP_TRY(t.alloc(&p, n * dim * 4));
        HIP_TRY(hipMemcpy(p, data, n * dim * 4, hipMemcpyHostToDevice));
        d_data = p;
    }
    std::vector<float> h_cent;
    const float* cent_host = centroids;
    if (is_device_pointer(centroids)) {
        h_cent.resize(k * dim);
        HIP_TRY(hipMemcpy(h_cent.data(), centroids, k * dim * 4, hipMemcpyDeviceToHost));
        cent_host = h_cent.data();
    }
    uint32_t *d_lists = nullptr, *d_counts = nullptr, *d_off = nullptr, *d_pl = nullptr, *d_pv = nullptr;
    HIP_TRY(t.alloc(&d_lists, n * M * 4));
    HIP_TRY(t.alloc(&d_counts, n * 4));
    ClosureArgs a{};
    a.centroids = centroids; a.k = k; a.dim = dim; a.data = d_data; a.n = n; a.epsilon = epsilon; a.max_replicas = M;
    a.max_chunk_rows = max_chunk_rows; a.out_lists = d_lists; a.out_counts = d_counts;
    if ((rc = run_closure(a, dev, true))) return rc;
    std::vector<uint32_t> off(n);
    HIP_TRY(hipMemcpy(off.data(), d_counts, n * 4, hipMemcpyDeviceToHost));
    uint64_t pairs = 0;
    for (uint64_t i = 0; i < n; ++i) { const uint32_t c = off[i]; off[i] = (uint32_t)pairs; pairs += c; }
    if (pairs > 0xfffffff0ull) return fail(RBQ_INVALID_CONFIG, "too many (vector, list) pairs for 32-bit slots");
    HIP_TRY(t.alloc(&d_off, n * 4));
    HIP_TRY(t.alloc(&d_pl, pairs * 4));
    HIP_TRY(t.alloc(&d_pv, pairs * 4));
    HIP_TRY(hipMemcpy(d_off, off.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_closure_expand(d_lists, d_counts, d_off, n, M, d_pl, d_pv, 0));
    HIP_TRY(hipDeviceSynchronize());
    return build_device_pairs(hdr, cent_host, d_data, d_pl, d_pv, pairs, rescale, t_const, dev, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_mstg_closure_assign(const float* centroids, uint64_t n_lists, uint32_t dim, const float* data, uint64_t n, float epsilon,
                            uint32_t max_replicas, uint64_t max_chunk_rows, int device, uint32_t* out_lists, uint32_t* out_counts) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    int rc = check_closure_args(centroids, n_lists, dim, data, n, epsilon, max_replicas);
    if (rc) return rc;
    if (!out_lists || !out_counts) return fail(RBQ_INVALID_CONFIG, "null buffer");
    std::vector<int> devs;
    if ((rc = resolve_devices(1, device < 0 ? nullptr : &device, devs))) return rc;
    DeviceGuard g(devs[0]);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    ClosureArgs a{};
    a.centroids = centroids; a.k = n_lists; a.dim = dim; a.data = data; a.n = n; a.epsilon = epsilon; a.max_replicas = max_replicas;
    a.max_chunk_rows = max_chunk_rows; a.out_lists = out_lists; a.out_counts = out_counts;
    return run_closure(a, devs[0], true);
    RBQ_GUARD_END
}

int rbq_mstg_build_device(const rbq_header* hdr, const float* centroids, const float* data, uint64_t n, float closure_epsilon,
                          uint32_t max_replicas, int rescale, float t_const, uint64_t max_chunk_rows, int device, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return build_impl(hdr, centroids, data, n, closure_epsilon, max_replicas, rescale, t_const, max_chunk_rows, device, out);
    RBQ_GUARD_END
}

int rbq_mstg_cluster_device(const float* data, uint64_t n, uint32_t dim, uint64_t max_posting_size, uint64_t branching_factor,
                            float balance_weight, uint64_t max_iterations, uint64_t host_below, int device, rbq_hclustered** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (const char* why = rbq_host::hc_check(data, n, dim, max_posting_size, branching_factor, max_iterations))
        return fail(RBQ_INVALID_CONFIG, why);
    std::vector<int> devs;
    int rc;
    if ((rc = resolve_devices(1, device < 0 ? nullptr : &device, devs))) return rc;
    DeviceGuard g(devs[0]);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    Scratch t;
    HClusterArgs a{};
    a.n = n; a.dim = dim; a.max_size = max_posting_size; a.k = branching_factor; a.niter = max_iterations;
    a.balance_weight = balance_weight; a.device = devs[0];
    a.host_below = host_below == RBQ_MSTG_HOST_BELOW_DEFAULT ? RBQ_MSTG_HOST_BELOW : host_below;
    if (is_device_pointer(data)) {
        a.d_data = data;
    } else {   // uploaded once
        float* p = nullptr;
        HIP_TRY(t.alloc(&p, n * dim * 4));
        HIP_TRY(hipMemcpy(p, data, n * dim * 4, hipMemcpyHostToDevice));
        a.d_data = p;
        a.h_data = data;
    }
    std::unique_ptr<rbq_hclustered> h(new rbq_hclustered());
    std::string detail;
    if ((rc = hcluster_device(a, h->r, detail))) return fail(rc, detail);
    *out = h.release();
    return RBQ_OK;
    RBQ_GUARD_END
}
uint64_t rbq_hclustered_count(const rbq_hclustered* h) { return h->r.offsets.size() - 1; }
const float* rbq_hclustered_centroids(const rbq_hclustered* h) { return h->r.centroids.data(); }
const uint64_t* rbq_hclustered_offsets(const rbq_hclustered* h) { return h->r.offsets.data(); }
const uint32_t* rbq_hclustered_members(const rbq_hclustered* h) { return h->r.members.data(); }
const uint64_t* rbq_hclustered_stats(const rbq_hclustered* h) { return h->r.stats; }
void rbq_hclustered_free(rbq_hclustered* h) { delete h; }

uint64_t rbq_mstg_debug_closure_fallbacks(void) { return g_closure_fallbacks.load(std::memory_order_relaxed); }

int rbq_mstg_debug_closure_shortlist(const float* centroids, uint64_t n_lists, uint32_t dim, const float* data, uint64_t n,
                                     uint32_t max_replicas, uint64_t max_chunk_rows, int device, uint32_t* out_sl, uint32_t* out_sl_n) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    int rc = check_closure_args(centroids, n_lists, dim, data, n, 0.0f, max_replicas);
    if (rc) return rc;
    if (!out_sl || !out_sl_n) return fail(RBQ_INVALID_CONFIG, "null buffer");
    std::vector<int> devs;
    if ((rc = resolve_devices(1, device < 0 ? nullptr : &device, devs))) return rc;
    DeviceGuard g(devs[0]);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    ClosureArgs a{};
    a.centroids = centroids; a.k = n_lists; a.dim = dim; a.data = data; a.n = n; a.max_replicas = max_replicas;
    a.max_chunk_rows = max_chunk_rows; a.tap_sl = out_sl; a.tap_sl_n = out_sl_n;
    return run_closure(a, devs[0], false);
    RBQ_GUARD_END
}
} // extern "C"
