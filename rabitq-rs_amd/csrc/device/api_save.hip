// api_save.hip — RBQ1 writer: save_to_writer, src/ivf.rs:1310-1474.
#include "api.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
constexpr uint64_t kSaveChunkBytes = 64ull << 20; // staging chunk (the load path's bound)

// words of every cluster in the cluster section (src/ivf.rs:1415-1466): centroid | n | ids | batch_data_len | batch_data |
// n x (len | ex code) | f_add_ex | f_rescale_ex | delta | vl
void save_layout(const Replica* ix, std::vector<uint64_t>& woff) {
    const uint64_t D = ix->D, exw = D * ix->ex_bits / 32;
    woff.assign(ix->n_lists + 1, 0);
    for (uint64_t c = 0; c < ix->n_lists; ++c) {
        const uint64_t n = ix->h_list_n[c], nb = (n + 31) / 32;
        woff[c + 1] = woff[c] + D + 4 + 2 * n + nb * (D + 96) + n * (2 + exw) + 4 * n;
    }
}

int save_check(const rbq_index* h) {
    if (!h || h->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    const Replica* ix = h->reps[0];
    if (ix->rotator == RBQ_ROTATOR_NONE)
        return fail(RBQ_INVALID_CONFIG, "posting-list handles (RBQ_ROTATOR_NONE) have no RBQ1 rotator tag and cannot be saved");
    if (!ix->has_recon)
        return fail(RBQ_INVALID_CONFIG, "the index holds no reconstruction factors (delta / vl): it was made by rbq_index_create; "
                                        "use rbq_index_create_with_recon, rbq_index_load_rbq1 or a device encoder");
    return RBQ_OK;
}

uint64_t save_total_bytes(const Replica* ix) {
    std::vector<uint64_t> woff;
    save_layout(ix, woff);
    return 44 + ix->rot_blob.bytes + woff.back() * 4 + 4;
}

int save_impl(const rbq_index* h, rbq_write_fn write, void* user) {
    int rc = save_check(h);
    if (rc) return rc;
    if (!write) return fail(RBQ_INVALID_CONFIG, "null writer");
    const Replica* ix = h->reps[0];
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    const uint64_t rot_len = ix->rot_blob.bytes;
    std::vector<uint64_t> woff;
    save_layout(ix, woff);
    const uint64_t total_w = woff.back();

    Scratch R; // everything a save allocates, freed on every exit (the handle itself is only read)
    hipEvent_t ev[2];
    uint8_t* pin[2];
    HIP_TRY(R.make_stream());
    for (auto& e : ev) HIP_TRY(R.event(&e));
    uint64_t chunk_w = (ix->opt.save_chunk ? ix->opt.save_chunk : kSaveChunkBytes) / 4;
    chunk_w = std::max<uint64_t>(1, std::min<uint64_t>(chunk_w, std::max<uint64_t>(total_w, 1)));
    const uint64_t chunk_b = chunk_w * 4;
    uint64_t* d_woff = nullptr;
    uint32_t *d_seg = nullptr, *d_crc = nullptr;
    uint8_t* d_stage[2] = {nullptr, nullptr};
    HIP_TRY(R.alloc(&d_woff, woff.size() * 8));
    HIP_TRY(R.alloc(&d_seg, std::max(crc_scratch_words(chunk_b), crc_scratch_words(rot_len)) * 4));
    HIP_TRY(R.alloc(&d_crc, 3 * 4)); // [0], [1]: chunk CRC of buffer 0 / 1; [2]: rotator
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(R.alloc(&d_stage[i], chunk_b));
        HIP_TRY(R.alloc_pinned(&pin[i], chunk_b + 4));
    }
    HIP_TRY(hipMemcpyAsync(d_woff, woff.data(), woff.size() * 8, hipMemcpyHostToDevice, R.stream));

    // header and rotator (save_to_writer: magic, version, then the hashed fields)
    std::vector<uint8_t> head(44 + rot_len); // magic, version, 36 hashed header bytes, rotator
    {
        uint8_t* o = head.data();
        auto put = [&](const void* p, size_t n) { std::memcpy(o, p, n); o += n; };
        const uint32_t version = 3, dim = ix->dim, D = ix->D;
        const uint8_t tags[4] = {ix->metric, ix->rotator, ix->ex_bits, (uint8_t)(ix->ex_bits + 1)};
        const uint64_t nv = ix->n_vectors, nl = ix->n_lists;
        put("RBQ1", 4); put(&version, 4); put(&dim, 4); put(&D, 4); put(tags, 4); put(&nv, 8); put(&nl, 8); put(&rot_len, 8);
    }
    uint32_t crc = rbq_host::crc32_update(0, head.data() + 8, 36);
    if (rot_len) {
        HIP_TRY(hipMemcpyAsync(head.data() + 44, ix->rot_blob.p, rot_len, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(launch_crc32((const uint8_t*)ix->rot_blob.p, rot_len, d_seg, d_crc + 2, R.stream));
        uint32_t rot_crc = 0;
        HIP_TRY(hipMemcpyAsync(&rot_crc, d_crc + 2, 4, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipStreamSynchronize(R.stream));
        crc = rbq_host::crc32_combine(crc, rot_crc, rot_len);
    }
    if (write(user, head.data(), head.size()) != 0) return fail(RBQ_IO, "the writer failed (header)");

    SaveParams P;
    P.woff = d_woff; P.list_gb0 = (const uint32_t*)ix->list_gb0.p; P.list_n = (const uint32_t*)ix->list_n.p;
    P.centroids = (const float*)ix->centroids.p; P.blocks = (const uint8_t*)ix->blocks.p; P.ids = (const uint64_t*)ix->ids.p;
    P.ex = (const uint8_t*)ix->ex.p; P.fadd_ex = (const float*)ix->fadd_ex.p; P.fres_ex = (const float*)ix->fres_ex.p;
    P.delta = (const float*)ix->delta.p; P.vl = (const float*)ix->vl.p;
    P.exd = ex_bytes_dev(ix->D, ix->ex_bits); P.n_lists = (uint32_t)ix->n_lists; P.D = ix->D; P.Dc = ix->Dc; P.ex_bits = ix->ex_bits;
    P.ex_words = ix->D * ix->ex_bits / 32; P.cpu = ex_cpu(ix->ex_bits);

    // double-buffered chunks: the kernels fill chunk i + 1 (and its copy runs) while the writer takes chunk i
    const uint64_t nchunks = (total_w + chunk_w - 1) / chunk_w;
    auto issue = [&](uint64_t k) -> int {
        const int b = (int)(k & 1);
        const uint64_t w0 = k * chunk_w, nw = std::min(chunk_w, total_w - w0);
        HIP_TRY(launch_save_fill(P, w0, nw, (uint32_t*)d_stage[b], R.stream));
        HIP_TRY(launch_crc32(d_stage[b], nw * 4, d_seg, d_crc + b, R.stream));
        HIP_TRY(hipMemcpyAsync(pin[b], d_stage[b], nw * 4, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipMemcpyAsync((uint8_t*)pin[b] + chunk_b, d_crc + b, 4, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipEventRecord(ev[b], R.stream));
        return RBQ_OK;
    };
    if (nchunks && (rc = issue(0))) return rc;
    for (uint64_t k = 0; k < nchunks; ++k) {
        if (k + 1 < nchunks && (rc = issue(k + 1))) return rc;
        const int b = (int)(k & 1);
        HIP_TRY(hipEventSynchronize(ev[b]));
        const uint64_t nb = std::min(chunk_w, total_w - k * chunk_w) * 4;
        uint32_t ccrc;
        std::memcpy(&ccrc, (const uint8_t*)pin[b] + chunk_b, 4);
        crc = rbq_host::crc32_combine(crc, ccrc, nb);
        if (write(user, pin[b], nb) != 0) return fail(RBQ_IO, "the writer failed (chunk " + std::to_string(k) + ")");
    }
    if (write(user, &crc, 4) != 0) return fail(RBQ_IO, "the writer failed (checksum)");
    HIP_TRY(hipStreamSynchronize(R.stream));
    return RBQ_OK;
}

struct BufSink { uint8_t* p; uint64_t cap, len; };
int buf_sink(void* user, const void* bytes, uint64_t len) {
    BufSink* s = (BufSink*)user;
    if (s->len + len > s->cap) return 1;
    std::memcpy(s->p + s->len, bytes, len);
    s->len += len;
    return 0;
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_index_save_rbq1_stream(const rbq_index* idx, rbq_write_fn write, void* user) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return save_impl(idx, write, user);
    RBQ_GUARD_END
}

int rbq_index_save_rbq1(const rbq_index* idx, uint8_t** bytes, uint64_t* len) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!bytes || !len) return fail(RBQ_INVALID_CONFIG, "null output");
    *bytes = nullptr; *len = 0;
    int rc = save_check(idx);
    if (rc) return rc;
    const uint64_t total = save_total_bytes(idx->reps[0]);
    BufSink sink{(uint8_t*)std::malloc(total ? total : 1), total, 0};
    if (!sink.p) return fail(RBQ_IO, "out of host memory");
    rc = save_impl(idx, buf_sink, &sink);
    if (rc == RBQ_OK && sink.len != total) rc = fail(RBQ_IO, "internal error: stream length");
    if (rc) { std::free(sink.p); return rc; }
    *bytes = sink.p; *len = total;
    return RBQ_OK;
    RBQ_GUARD_END
}

void rbq_persist_free_bytes(uint8_t* bytes) { std::free(bytes); }
} // extern "C"
