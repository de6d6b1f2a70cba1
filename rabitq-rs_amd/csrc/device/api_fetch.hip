// api_fetch.hip — fetch_embedding: IvfRabitqIndex::fetch_embedding, src/ivf.rs:1247-1307.
// Served from the first replica (it keeps delta / vl).  The id map is built once, on the first fetch; each call then runs
// k_fetch_vec (and k_fetch_matrix for the Matrix rotator) on its own or the caller's stream.  A fetch only reads the index.
#include "api.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
constexpr uint64_t kFetchChunkBytes = 64ull << 20; // host entry: output staging per chunk; Matrix rotator: rotated-row scratch

int fetch_check(const rbq_index* h) {
    if (!h || h->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    const Replica* ix = h->reps[0];
    if (ix->rotator == RBQ_ROTATOR_NONE)
        return fail(RBQ_INVALID_CONFIG, "posting-list handles (RBQ_ROTATOR_NONE) have no rotator to invert");
    if (!ix->has_recon)
        return fail(RBQ_INVALID_CONFIG, "the index holds no reconstruction factors (delta / vl): it was made by rbq_index_create; "
                                        "use rbq_index_create_with_recon, rbq_index_load_rbq1 or a device encoder");
    return RBQ_OK;
}

// The id map of the first replica, built on first use (the caller has switched to its device).  Blocks until it is built.
int fetch_map(Replica* ix) {
    std::lock_guard<std::mutex> lk(ix->fetch_mu);
    if (ix->fmap_ready) return RBQ_OK;
    const uint64_t n = ix->n_vectors, nl = ix->n_lists;
    std::vector<uint64_t> vstart(nl + 1, 0);
    for (uint64_t c = 0; c < nl; ++c) vstart[c + 1] = vstart[c] + ix->h_list_n[c];
    if (vstart[nl] != n) return fail(RBQ_IO, "internal error: list sizes do not add up to the vector count");
    Arr ids, slots;
    struct Keep { Arr *a, *b; ~Keep() { for (Arr* x : {a, b}) if (x->p) (void)hipFree(x->p); } } keep{&ids, &slots};
    int rc;
    if ((rc = alloc_arr(ids, n * 8))) return rc;
    if ((rc = alloc_arr(slots, n * 4))) return rc;
    if (n) {
        Scratch t;
        HIP_TRY(t.make_stream());
        const hipStream_t st = t.stream;
        uint64_t* d_vstart = nullptr;
        uint64_t* d_kin = nullptr;
        uint32_t* d_vin = nullptr;
        void* d_tmp = nullptr;
        size_t tb = 0;
        HIP_TRY(sort_pairs_u64_u32(nullptr, &tb, nullptr, nullptr, nullptr, nullptr, (size_t)n, st));
        HIP_TRY(t.alloc(&d_vstart, (nl + 1) * 8));
        HIP_TRY(t.alloc(&d_kin, n * 8));
        HIP_TRY(t.alloc(&d_vin, n * 4));
        HIP_TRY(t.alloc(&d_tmp, tb));
        HIP_TRY(hipMemcpyAsync(d_vstart, vstart.data(), (nl + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_fetch_gather(d_vstart, (const uint32_t*)ix->list_gb0.p, (uint32_t)nl, (const uint64_t*)ix->ids.p, n, d_kin, d_vin, st));
        HIP_TRY(sort_pairs_u64_u32(d_tmp, &tb, d_kin, (uint64_t*)ids.p, d_vin, (uint32_t*)slots.p, (size_t)n, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    ix->fmap_ids = ids; ix->fmap_slots = slots;
    ids = Arr(); slots = Arr();
    ix->fmap_ready = true;
    return RBQ_OK;
}

FetchParams fetch_params(const Replica* ix) {
    FetchParams P;
    P.map_ids = (const uint64_t*)ix->fmap_ids.p; P.map_slots = (const uint32_t*)ix->fmap_slots.p; P.n_map = ix->n_vectors;
    P.list_gb0 = (const uint32_t*)ix->list_gb0.p; P.centroids = (const float*)ix->centroids.p; P.blocks = (const uint8_t*)ix->blocks.p;
    P.ex = (const uint8_t*)ix->ex.p; P.delta = (const float*)ix->delta.p; P.vl = (const float*)ix->vl.p;
    P.rot_blob = (const uint8_t*)ix->rot_blob.p; P.exd = ex_bytes_dev(ix->D, ix->ex_bits);
    P.n_lists = (uint32_t)ix->n_lists; P.dim = ix->dim; P.D = ix->D; P.Dc = ix->Dc; P.ex_bits = ix->ex_bits; P.cpu = ex_cpu(ix->ex_bits);
    P.rotator = ix->rotator; P.trunc = ix->trunc;
    // the crate's f32 divisions 1.0 / self.fac and 1.0 / (n as f32), n the FHT's length: padded_dim when trunc_dim == padded_dim,
    // else trunc_dim — trunc_dim in both cases
    P.rfac = 1.0f / ix->fac;
    P.rlen = 1.0f / (float)ix->trunc;
    return P;
}

// ids per Matrix launch: the rotated-row scratch stays within kFetchChunkBytes
uint64_t fetch_matrix_rows(const Replica* ix) { return std::max<uint64_t>(1, kFetchChunkBytes / ((uint64_t)ix->D * 4)); }

int fetch_host_impl(const rbq_index* h, const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
    int rc = fetch_check(h);
    if (rc) return rc;
    if (n == 0) return RBQ_OK;
    if (!ids || !out || !found) return fail(RBQ_INVALID_CONFIG, "null ids / out / found");
    Replica* ix = h->reps[0];
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    if ((rc = fetch_map(ix))) return rc;
    const FetchParams P = fetch_params(ix);
    const uint64_t dim = ix->dim, D = ix->D;
    const bool matrix = ix->rotator != RBQ_ROTATOR_FHT_KAC;
    uint64_t chunk = ix->opt.fetch_chunk ? ix->opt.fetch_chunk : std::max<uint64_t>(1, kFetchChunkBytes / (dim * 4 + 9));
    if (matrix) chunk = std::min(chunk, fetch_matrix_rows(ix));
    chunk = std::min(chunk, n);
    // page-locked staging, per buffer: ids [chunk] u64 | out [chunk][dim] f32 | found [chunk] u8
    const size_t o_out = chunk * 8, o_found = o_out + chunk * dim * 4, pin_b = o_found + chunk;
    Scratch R; // everything a host-entry fetch allocates, freed on every exit
    hipEvent_t ev[2];
    uint8_t* pin[2];
    HIP_TRY(R.make_stream());
    for (auto& e : ev) HIP_TRY(R.event(&e));
    uint8_t* d_buf[2] = {nullptr, nullptr};
    float* d_rows = nullptr;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(R.alloc(&d_buf[i], pin_b));
        HIP_TRY(R.alloc_pinned(&pin[i], pin_b));
    }
    if (matrix) HIP_TRY(R.alloc(&d_rows, chunk * D * 4)); // one stream: the chunks' launches never overlap
    const uint64_t nchunks = (n + chunk - 1) / chunk;
    auto issue = [&](uint64_t k) -> int {
        const int b = (int)(k & 1);
        const uint64_t k0 = k * chunk, m = std::min(chunk, n - k0);
        uint8_t* hp = pin[b];
        uint8_t* dp = d_buf[b];
        std::memcpy(hp, ids + k0, m * 8);
        HIP_TRY(hipMemcpyAsync(dp, hp, m * 8, hipMemcpyHostToDevice, R.stream));
        HIP_TRY(launch_fetch(P, (const uint64_t*)dp, m, (float*)(dp + o_out), dp + o_found, d_rows, R.stream));
        HIP_TRY(hipMemcpyAsync(hp + o_out, dp + o_out, m * dim * 4, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipMemcpyAsync(hp + o_found, dp + o_found, m, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipEventRecord(ev[b], R.stream));
        return RBQ_OK;
    };
    // double-buffered: chunk k + 1 is staged and enqueued while the host copies chunk k out
    if ((rc = issue(0))) return rc;
    for (uint64_t k = 0; k < nchunks; ++k) {
        if (k + 1 < nchunks && (rc = issue(k + 1))) return rc;
        const int b = (int)(k & 1);
        HIP_TRY(hipEventSynchronize(ev[b]));
        const uint64_t k0 = k * chunk, m = std::min(chunk, n - k0);
        const uint8_t* hp = pin[b];
        std::memcpy(out + k0 * dim, hp + o_out, m * dim * 4);
        std::memcpy(found + k0, hp + o_found, m);
    }
    return RBQ_OK;
}

int fetch_device_impl(const rbq_index* h, const uint64_t* d_ids, uint64_t n, float* d_out, uint8_t* d_found, hipStream_t s) {
    int rc = fetch_check(h);
    if (rc) return rc;
    if (n == 0) return RBQ_OK;
    if (!d_ids || !d_out || !d_found) return fail(RBQ_INVALID_CONFIG, "null ids / out / found");
    Replica* ix = h->reps[0];
    {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, d_ids) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RBQ_INVALID_CONFIG, "d_ids is not device memory");
        }
        if (a.type != hipMemoryTypeDevice || a.device != ix->device)
            return fail(RBQ_INVALID_CONFIG, "d_ids must be device memory of the first replica's device (" + std::to_string(ix->device) + ")");
    }
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    if ((rc = fetch_map(ix))) return rc;
    const FetchParams P = fetch_params(ix);
    if (ix->rotator == RBQ_ROTATOR_FHT_KAC) {
        HIP_TRY(launch_fetch(P, d_ids, n, d_out, d_found, nullptr, s));
        return RBQ_OK;
    }
    // Matrix: rotated rows through a stream-ordered scratch, a bounded number of ids per launch
    const uint64_t rows = std::min(n, fetch_matrix_rows(ix));
    float* d_rows = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d_rows, rows * ix->D * 4, s));
    for (uint64_t k0 = 0; k0 < n; k0 += rows) {
        const uint64_t m = std::min(rows, n - k0);
        const hipError_t e = launch_fetch(P, d_ids + k0, m, d_out + k0 * ix->dim, d_found + k0, d_rows, s);
        if (e != hipSuccess) {
            (void)hipFreeAsync(d_rows, s);
            return fail(RBQ_DEVICE, std::string("launch_fetch: ") + hipGetErrorString(e));
        }
    }
    HIP_TRY(hipFreeAsync(d_rows, s));
    return RBQ_OK;
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_index_fetch_embeddings(const rbq_index* idx, const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return fetch_host_impl(idx, ids, n, out, found);
    RBQ_GUARD_END
}

int rbq_index_fetch_embeddings_device(const rbq_index* idx, const uint64_t* d_ids, uint64_t n, float* d_out, uint8_t* d_found,
                                      void* hip_stream) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return fetch_device_impl(idx, d_ids, n, d_out, d_found, (hipStream_t)hip_stream);
    RBQ_GUARD_END
}
} // extern "C"
