// api_bf_mutate.hip — rbq_bf_append, rbq_bf_remove_ids, rbq_bf_fetch_embeddings* (include/rbq_bf_mutate.h):
// new handles that hold a brute-force index's vectors and `count` more, or all but those at a set of positions, and
// fetch_embedding from the flat layout.  Nothing old is encoded again: an append carries the old arrays by device-to-device
// copies and runs the trainer's encoder chain (bf_encode_rows, api_bf.hip) over the new rows at their offsets; a removal is a
// stream compaction of the flat arrays (k_bf_mutate.hip).  The input handle is only read.
#include "bf_index.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
constexpr uint64_t kBfFetchChunkBytes = 64ull << 20; // host entry: ids + rows + flags of one chunk; Matrix rotator: rotated-row scratch
std::atomic<uint64_t> g_bf_carry_ns{0};  // rbq_bf_debug_append_carry_ns: device time of the last append's carry copies
std::atomic<uint64_t> g_bf_gather_ns{0}; // rbq_bf_debug_remove_gather_ns: device time of the last gather kernel

int bf_append_impl(const rbq_bf_index* old, const float* vectors, uint64_t count, int rescale, float t_const, uint64_t max_chunk_rows,
                   rbq_bf_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null output");
    *out = nullptr;
    if (!old) return fail(RBQ_INVALID_CONFIG, "null index");
    if (!vectors) return fail(RBQ_INVALID_CONFIG, "null vectors");
    if (count == 0) return fail(RBQ_INVALID_CONFIG, "no vectors to append");
    const uint64_t len = old->hdr.n_vectors;
    if (count > 0xffffffffull || len + count > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "more than 2^32 vectors");
    const int opt = rescale_mode(rescale, &old->hdr);
    if (opt < 0) return RBQ_INVALID_CONFIG;
    if (!opt && old->hdr.ex_bits > 0 && !(t_const > 0.0f))
        return fail(RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)");
    DeviceGuard g(old->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    int rc;
    BfOwner own{nullptr};
    if ((rc = bf_new_index(&old->hdr, len + count, old->ex_len, old->device, own))) return rc;
    rbq_bf_index* ix = own.ix;
    {
        EventPair ev;
        ev.start();
        if (old->bin.bytes) HIP_TRY(hipMemcpyAsync(ix->bin.p, old->bin.p, old->bin.bytes, hipMemcpyDeviceToDevice, 0));
        if (old->ex.bytes) HIP_TRY(hipMemcpyAsync(ix->ex.p, old->ex.p, old->ex.bytes, hipMemcpyDeviceToDevice, 0));
        for (int k = 0; k < 8; ++k)
            if (old->f[k].bytes) HIP_TRY(hipMemcpyAsync(ix->f[k].p, old->f[k].p, old->f[k].bytes, hipMemcpyDeviceToDevice, 0));
        ev.stop();
        uint64_t ns = 0;
        if (ev.ns(&ns)) g_bf_carry_ns.store(ns, std::memory_order_relaxed);
    }
    if ((rc = bf_encode_rows(ix, vectors, count, len, opt != 0, t_const, max_chunk_rows))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = own.release();
    return RBQ_OK;
}

int bf_remove_impl(const rbq_bf_index* old, const uint64_t* ids, uint64_t n_ids, uint64_t* out_removed, rbq_bf_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null output");
    *out = nullptr;
    if (!old) return fail(RBQ_INVALID_CONFIG, "null index");
    if (!ids) return fail(RBQ_INVALID_CONFIG, "null ids");
    if (n_ids == 0) return fail(RBQ_INVALID_CONFIG, "no ids");
    const uint64_t n = old->hdr.n_vectors;
    if (n == 0) return fail(RBQ_EMPTY_INDEX, "index is empty");
    DeviceGuard g(old->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    int rc;
    Scratch tm; // the row map: lives until the gather has run
    uint32_t* d_map = nullptr;
    uint64_t kept = 0;
    {
        // ---- mark and rank: freed again before the new arrays are allocated
        Scratch t;
        const uint64_t* d_in = ids;
        if (!is_device_pointer(ids)) {
            uint64_t* p = nullptr;
            HIP_TRY(t.alloc(&p, n_ids * 8));
            HIP_TRY(hipMemcpy(p, ids, n_ids * 8, hipMemcpyHostToDevice));
            d_in = p;
        }
        uint8_t* d_keep = nullptr;
        uint32_t* d_rank = nullptr;
        void* d_tmp = nullptr;
        size_t tb = 0;
        HIP_TRY(t.alloc(&d_keep, n + 1)); // (one entry more, 0: the scan's last value is the total)
        HIP_TRY(t.alloc(&d_rank, (n + 1) * 4));
        HIP_TRY(hipMemsetAsync(d_keep, 1, n, 0));
        HIP_TRY(hipMemsetAsync(d_keep + n, 0, 1, 0));
        HIP_TRY(launch_bf_mark(d_in, n_ids, n, d_keep, 0));
        HIP_TRY(bf_scan_kept(nullptr, &tb, d_keep, d_rank, n + 1, 0));
        HIP_TRY(t.alloc(&d_tmp, tb));
        HIP_TRY(bf_scan_kept(d_tmp, &tb, d_keep, d_rank, n + 1, 0));
        uint32_t k32 = 0;
        HIP_TRY(hipMemcpy(&k32, d_rank + n, 4, hipMemcpyDeviceToHost));
        kept = k32;
        if (kept > n) return fail(RBQ_IO, "internal error: more survivors than vectors");
        if (kept == 0) // (rbq_bf_train_device refuses zero rows too: there is no trained handle without vectors)
            return fail(RBQ_INVALID_CONFIG, "the ids cover every vector of the index: an index without vectors cannot be built");
        HIP_TRY(tm.alloc(&d_map, kept * 4));
        HIP_TRY(launch_bf_row_map(d_keep, d_rank, n, d_map, 0));
        HIP_TRY(hipDeviceSynchronize());
    }
    BfOwner own{nullptr};
    if ((rc = bf_new_index(&old->hdr, kept, old->ex_len, old->device, own))) return rc;
    rbq_bf_index* ix = own.ix;
    {
        BfGatherParams P{};
        P.map = d_map; P.n_new = kept; P.n_old = n;
        P.bin_len = old->D / 8; P.ex_len = old->ex.bytes ? old->D * old->ex_bits / 8 : 0;
        P.bin_s = (const uint8_t*)old->bin.p; P.bin_d = (uint8_t*)ix->bin.p;
        P.ex_s = (const uint8_t*)old->ex.p; P.ex_d = (uint8_t*)ix->ex.p;
        for (int k = 0; k < 8; ++k) { P.f_s[k] = (const float*)old->f[k].p; P.f_d[k] = (float*)ix->f[k].p; }
        EventPair ev;
        ev.start();
        HIP_TRY(launch_bf_gather(P, old->device, 0));
        ev.stop();
        uint64_t ns = 0;
        if (ev.ns(&ns)) g_bf_gather_ns.store(ns, std::memory_order_relaxed);
    }
    HIP_TRY(hipDeviceSynchronize());
    if (out_removed) *out_removed = n - kept;
    *out = own.release();
    return RBQ_OK;
}

BfFetchParams bf_fetch_params(const rbq_bf_index* ix) {
    BfFetchParams P;
    P.bin = (const uint8_t*)ix->bin.p; P.ex = (const uint8_t*)ix->ex.p; P.delta = (const float*)ix->f[0].p; P.vl = (const float*)ix->f[1].p;
    P.rot_blob = (const uint8_t*)ix->rot_blob.p; P.n_vectors = ix->hdr.n_vectors;
    P.dim = ix->dim; P.D = ix->D; P.ex_bits = ix->ex_bits; P.rotator = ix->rotator; P.trunc = ix->trunc;
    // the crate's f32 divisions 1.0 / self.fac and 1.0 / (n as f32), n the FHT's length (api_fetch.hip)
    P.rfac = 1.0f / ix->fac;
    P.rlen = 1.0f / (float)ix->trunc;
    return P;
}

int bf_fetch_host_impl(const rbq_bf_index* ix, const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
    if (!ix) return fail(RBQ_INVALID_CONFIG, "null index");
    if (n == 0) return RBQ_OK;
    if (!ids || !out || !found) return fail(RBQ_INVALID_CONFIG, "null ids / out / found");
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    const BfFetchParams P = bf_fetch_params(ix);
    const uint64_t dim = ix->dim, D = ix->D;
    const bool matrix = ix->rotator != RBQ_ROTATOR_FHT_KAC;
    // one chunk: ids [chunk] u64 | out [chunk][dim] f32 | found [chunk] u8 (and the Matrix rotator's rotated rows) within the budget
    const uint64_t chunk = std::min(n, std::max<uint64_t>(1, kBfFetchChunkBytes / (dim * 4 + 9 + (matrix ? D * 4 : 0))));
    Scratch t;
    HIP_TRY(t.make_stream());
    uint64_t* d_ids = nullptr;
    float *d_out = nullptr, *d_rows = nullptr;
    uint8_t* d_found = nullptr;
    HIP_TRY(t.alloc(&d_ids, chunk * 8));
    HIP_TRY(t.alloc(&d_out, chunk * dim * 4));
    HIP_TRY(t.alloc(&d_found, chunk));
    if (matrix) HIP_TRY(t.alloc(&d_rows, chunk * D * 4));
    for (uint64_t k0 = 0; k0 < n; k0 += chunk) {
        const uint64_t m = std::min(chunk, n - k0);
        HIP_TRY(hipMemcpyAsync(d_ids, ids + k0, m * 8, hipMemcpyHostToDevice, t.stream));
        HIP_TRY(launch_bf_fetch(P, d_ids, m, d_out, d_found, d_rows, t.stream));
        HIP_TRY(hipMemcpyAsync(out + k0 * dim, d_out, m * dim * 4, hipMemcpyDeviceToHost, t.stream));
        HIP_TRY(hipMemcpyAsync(found + k0, d_found, m, hipMemcpyDeviceToHost, t.stream));
        HIP_TRY(hipStreamSynchronize(t.stream)); // the chunk's buffers are reused
    }
    return RBQ_OK;
}

int bf_fetch_device_impl(const rbq_bf_index* ix, const uint64_t* d_ids, uint64_t n, float* d_out, uint8_t* d_found, hipStream_t s) {
    if (!ix) return fail(RBQ_INVALID_CONFIG, "null index");
    if (n == 0) return RBQ_OK;
    if (!d_ids || !d_out || !d_found) return fail(RBQ_INVALID_CONFIG, "null ids / out / found");
    {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, d_ids) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RBQ_INVALID_CONFIG, "d_ids is not device memory");
        }
        if (a.type != hipMemoryTypeDevice || a.device != ix->device)
            return fail(RBQ_INVALID_CONFIG, "d_ids must be device memory of the index's device (" + std::to_string(ix->device) + ")");
    }
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    const BfFetchParams P = bf_fetch_params(ix);
    if (ix->rotator == RBQ_ROTATOR_FHT_KAC) {
        HIP_TRY(launch_bf_fetch(P, d_ids, n, d_out, d_found, nullptr, s));
        return RBQ_OK;
    }
    // Matrix: rotated rows through a stream-ordered scratch, a bounded number of ids per launch
    const uint64_t rows = std::min(n, std::max<uint64_t>(1, kBfFetchChunkBytes / ((uint64_t)ix->D * 4)));
    float* d_rows = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d_rows, rows * ix->D * 4, s));
    for (uint64_t k0 = 0; k0 < n; k0 += rows) {
        const uint64_t m = std::min(rows, n - k0);
        const hipError_t e = launch_bf_fetch(P, d_ids + k0, m, d_out + k0 * ix->dim, d_found + k0, d_rows, s);
        if (e != hipSuccess) {
            (void)hipFreeAsync(d_rows, s);
            return fail(RBQ_DEVICE, std::string("launch_bf_fetch: ") + hipGetErrorString(e));
        }
    }
    HIP_TRY(hipFreeAsync(d_rows, s));
    return RBQ_OK;
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_bf_append(const rbq_bf_index* idx, const float* vectors, uint64_t count, int rescale, float t_const, uint64_t max_chunk_rows,
                  rbq_bf_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return bf_append_impl(idx, vectors, count, rescale, t_const, max_chunk_rows, out);
    RBQ_GUARD_END
}

int rbq_bf_remove_ids(const rbq_bf_index* idx, const uint64_t* ids, uint64_t n_ids, uint64_t* out_removed, rbq_bf_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return bf_remove_impl(idx, ids, n_ids, out_removed, out);
    RBQ_GUARD_END
}

int rbq_bf_fetch_embeddings(const rbq_bf_index* idx, const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return bf_fetch_host_impl(idx, ids, n, out, found);
    RBQ_GUARD_END
}

int rbq_bf_fetch_embeddings_device(const rbq_bf_index* idx, const uint64_t* d_ids, uint64_t n, float* d_out, uint8_t* d_found,
                                   void* hip_stream) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return bf_fetch_device_impl(idx, d_ids, n, d_out, d_found, (hipStream_t)hip_stream);
    RBQ_GUARD_END
}

uint64_t rbq_bf_debug_append_carry_ns(void) { return g_bf_carry_ns.load(std::memory_order_relaxed); }
uint64_t rbq_bf_debug_remove_gather_ns(void) { return g_bf_gather_ns.load(std::memory_order_relaxed); }
} // extern "C"
