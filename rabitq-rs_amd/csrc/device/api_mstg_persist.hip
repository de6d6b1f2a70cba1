// api_mstg_persist.hip — `.mstg` writer and loader (include/rbq_mstg_persist.h): MstgIndex::save_main_index / load_main_index,
// src/mstg/io.rs:129-245.  The framing is the host's (csrc/host/rbq_mstg_file.hpp); the records are assembled, taken apart,
// validated and checksummed by the GPU (k_mstg_save.hip, k_save.hip's CRC).
#include "api.hpp"
#include "rbq_mstg.h"
#include "../host/rbq_mstg_file.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
constexpr uint64_t kMstgChunkBytes = 64ull << 20; // staging chunk of the save, span budget of the load

int mstg_save_check(const rbq_index* h, const rbq_mstg_config* cfg) {
    if (!h || h->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    if (!cfg) return fail(RBQ_INVALID_CONFIG, "null config");
    const Replica* ix = h->reps[0];
    if (ix->rotator != RBQ_ROTATOR_NONE)
        return fail(RBQ_INVALID_CONFIG, "not an MSTG handle: only posting-list handles (RBQ_ROTATOR_NONE) are saved as .mstg");
    if (!ix->has_rnorm || !ix->has_recon)
        return fail(RBQ_INVALID_CONFIG, "the index holds no residual norms: it was made by rbq_index_create*; "
                                        "use rbq_mstg_build_device or rbq_mstg_load");
    if (const char* why = rbq_host::mstg_config_error(*cfg)) return fail(RBQ_INVALID_CONFIG, why);
    if (cfg->rabitq_bits != (uint64_t)ix->ex_bits + 1) return fail(RBQ_INVALID_CONFIG, "config: rabitq_bits disagrees with the handle");
    if (cfg->metric != ix->metric) return fail(RBQ_INVALID_CONFIG, "config: metric disagrees with the handle");
    return RBQ_OK;
}

// section offset of every list (its u64 length prefix); loff[n_lists] = the section's length
void mstg_layout(const Replica* ix, std::vector<uint64_t>& loff) {
    const uint64_t R = rbq_host::mstg_record_len(ix->D, ix->ex_bits);
    loff.assign(ix->n_lists + 1, 0);
    for (uint64_t c = 0; c < ix->n_lists; ++c) {
        const uint64_t n = ix->h_list_n[c];
        loff[c + 1] = loff[c] + 8 + rbq_host::mstg_list_header_len(ix->D, n && ix->tc_some) + n * R;
    }
}
uint64_t mstg_head_bytes(const Replica* ix) { return 8 + 8 + rbq_host::kMstgCfgBytes + 8 + 4 * ix->n_lists + 8; }

int mstg_save_impl(const rbq_index* h, const rbq_mstg_config* cfg, rbq_write_fn write, void* user) {
    int rc = mstg_save_check(h, cfg);
    if (rc) return rc;
    if (!write) return fail(RBQ_INVALID_CONFIG, "null writer");
    const Replica* ix = h->reps[0];
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    std::vector<uint64_t> loff;
    mstg_layout(ix, loff);
    const uint64_t total = loff.back();

    Scratch R; // everything a save allocates, freed on every exit (the handle itself is only read)
    hipEvent_t ev[2];
    uint8_t* pin[2];
    HIP_TRY(R.make_stream());
    for (auto& e : ev) HIP_TRY(R.event(&e));
    uint64_t chunk = ix->opt.mstg_chunk ? ix->opt.mstg_chunk : kMstgChunkBytes;
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, total));
    const uint64_t cap = align_up(chunk, 4);
    uint64_t* d_loff = nullptr;
    uint32_t *d_seg = nullptr, *d_crc = nullptr;
    uint8_t* d_stage[2] = {nullptr, nullptr};
    HIP_TRY(R.alloc(&d_loff, loff.size() * 8));
    HIP_TRY(R.alloc(&d_seg, crc_scratch_words(chunk) * 4));
    HIP_TRY(R.alloc(&d_crc, 2 * 4));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(R.alloc(&d_stage[i], cap));
        HIP_TRY(R.alloc_pinned(&pin[i], cap + 4));
    }
    HIP_TRY(hipMemcpyAsync(d_loff, loff.data(), loff.size() * 8, hipMemcpyHostToDevice, R.stream));

    // magic, version, then the hashed head: config, centroid ids, the number of lists
    std::vector<uint8_t> head(mstg_head_bytes(ix));
    {
        rbq_host::MstgPut p{head.data()};
        p.raw("MSTG", 4); p.u32(1);
        p.u64(rbq_host::kMstgCfgBytes);
        rbq_host::mstg_put_config(*cfg, p.o); p.o += rbq_host::kMstgCfgBytes;
        p.u64(ix->n_lists);
        for (uint64_t c = 0; c < ix->n_lists; ++c) p.u32((uint32_t)c);
        p.u64(ix->n_lists);
    }
    uint32_t crc = rbq_host::crc32_update(0, head.data() + 8, head.size() - 8);
    if (write(user, head.data(), head.size()) != 0) return fail(RBQ_IO, "the writer failed (header)");

    MstgSaveParams P;
    P.loff = d_loff; P.list_gb0 = (const uint32_t*)ix->list_gb0.p; P.list_n = (const uint32_t*)ix->list_n.p;
    P.centroids = (const float*)ix->centroids.p; P.blocks = (const uint8_t*)ix->blocks.p; P.ids = (const uint64_t*)ix->ids.p;
    P.ex = (const uint8_t*)ix->ex.p; P.fadd_ex = (const float*)ix->fadd_ex.p; P.fres_ex = (const float*)ix->fres_ex.p;
    P.delta = (const float*)ix->delta.p; P.vl = (const float*)ix->vl.p; P.rnorm = (const float*)ix->rnorm.p;
    P.exd = ex_bytes_dev(ix->D, ix->ex_bits); P.n_lists = (uint32_t)ix->n_lists; P.D = ix->D; P.Dc = ix->Dc; P.ex_bits = ix->ex_bits;
    P.cpu = ex_cpu(ix->ex_bits); P.has_t = ix->tc_some ? 1u : 0u;
    std::memcpy(&P.t_bits, &ix->tc_value, 4);
    P.R = (uint32_t)rbq_host::mstg_record_len(ix->D, ix->ex_bits); P.E = rbq_host::mstg_ex_len(ix->D, ix->ex_bits);

    // double-buffered chunks: the kernels fill chunk i + 1 (and its copy runs) while the writer takes chunk i
    const uint64_t nchunks = (total + chunk - 1) / chunk;
    auto issue = [&](uint64_t k) -> int {
        const int b = (int)(k & 1);
        const uint64_t b0 = k * chunk, nb = std::min(chunk, total - b0);
        HIP_TRY(launch_mstg_save_fill(P, b0, nb, (uint32_t*)d_stage[b], R.stream));
        HIP_TRY(launch_crc32(d_stage[b], nb, d_seg, d_crc + b, R.stream));
        HIP_TRY(hipMemcpyAsync(pin[b], d_stage[b], nb, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipMemcpyAsync((uint8_t*)pin[b] + cap, d_crc + b, 4, hipMemcpyDeviceToHost, R.stream));
        HIP_TRY(hipEventRecord(ev[b], R.stream));
        return RBQ_OK;
    };
    if (nchunks && (rc = issue(0))) return rc;
    for (uint64_t k = 0; k < nchunks; ++k) {
        if (k + 1 < nchunks && (rc = issue(k + 1))) return rc;
        const int b = (int)(k & 1);
        HIP_TRY(hipEventSynchronize(ev[b]));
        const uint64_t nb = std::min(chunk, total - k * chunk);
        uint32_t ccrc;
        std::memcpy(&ccrc, (const uint8_t*)pin[b] + cap, 4);
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

struct MemSrc { const uint8_t* p; uint64_t len; };
int mem_read(void* user, uint64_t off, void* dst, uint64_t n) {
    const MemSrc* m = (const MemSrc*)user;
    if (n > m->len || off > m->len - n) return 1;
    std::memcpy(dst, m->p + off, n);
    return 0;
}

// a span of the stream that goes to the device in one piece: whole list headers and whole blocks' records
struct Span { uint64_t a, e; uint32_t gb_first, nb; };

int mstg_load_impl(rbq_read_fn read, void* user, uint64_t total, int device, rbq_mstg_config* cfg_out, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (!read) return fail(RBQ_INVALID_CONFIG, "null reader");
    rbq_host::MstgFraming F;
    {
        std::string detail;
        auto rd = [&](uint64_t off, void* dst, uint64_t n) { return read(user, off, dst, n) == 0; };
        const int rc = rbq_host::mstg_parse_framing(rd, total, F, detail);
        if (rc) return fail(rc, detail);
    }
    const uint32_t D = F.D, ex_bits = F.ex_bits, nlist = (uint32_t)F.lists.size();
    rbq_header hdr;
    std::memset(&hdr, 0, sizeof hdr);
    hdr.dim = D; hdr.padded_dim = D; hdr.metric = (uint8_t)F.cfg.metric; hdr.rotator = RBQ_ROTATOR_NONE; hdr.ex_bits = (uint8_t)ex_bits;
    hdr.n_lists = nlist; hdr.n_vectors = F.n_vectors;
    int rc = validate_header(&hdr);
    if (rc) return rc;
    std::vector<int> devs;
    if ((rc = resolve_devices(1, device < 0 ? nullptr : &device, devs))) return rc;
    const int dev = devs[0];
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");

    ReplicaOwner own{new_replica(&hdr, dev)};
    Replica* ix = own.ix;
    Scratch t; // (released before `own`)
    const uint32_t Dc = ix->Dc;
    const uint64_t R = rbq_host::mstg_record_len(D, ex_bits);
    std::vector<uint32_t> ln(nlist);
    for (uint32_t c = 0; c < nlist; ++c) ln[c] = (uint32_t)F.lists[c].n;
    rbq_host::ListLayout lay;
    {   // (the framing has refused a stream whose lists pass 2^32 - 1 slots, with its own message)
        std::string detail;
        if (!rbq_host::list_layout(ln.data(), nlist, &lay, &detail)) return fail(RBQ_INVALID_PERSISTENCE, detail);
    }
    const std::vector<uint32_t>& gb0 = lay.gb0;
    const uint64_t nblocks = lay.blocks;
    if ((rc = upload_arr(ix->rot_blob, nullptr, 0))) return rc;
    if ((rc = upload_arr(ix->centroids, F.centroids.data(), F.centroids.size() * 4))) return rc;
    if ((rc = alloc_index_arrays(ix, ln, gb0, nblocks, F.n_vectors, /*recon=*/true, /*rnorm=*/true))) return rc;
    ix->tc_some = F.has_t; ix->tc_value = F.t_const;

    // block tables and the spans: units (a list's prefix and header, a block's records) are joined while they fit the budget
    std::vector<uint64_t> boff(nblocks);
    std::vector<uint32_t> bnv(nblocks);
    std::vector<Span> spans;
    // TEST ONLY: RBQ_MSTG_LOAD_SPAN in the environment (bytes) shrinks the budget — no handle exists yet to carry an option
    uint64_t budget = kMstgChunkBytes;
    if (const char* e = std::getenv("RBQ_MSTG_LOAD_SPAN")) { const long long v = std::atoll(e); if (v > 0) budget = (uint64_t)v; }
    uint64_t cap = 0;
    {
        Span cur{F.sec_begin, F.sec_begin, 0, 0};
        auto add = [&](uint64_t a, uint64_t e, uint32_t blocks, uint32_t gb) {
            if (cur.e > cur.a && e - cur.a > budget) { spans.push_back(cur); cur = Span{a, a, gb, 0}; }
            if (cur.e == cur.a) cur.gb_first = gb;
            cur.e = e; cur.nb += blocks;
        };
        for (uint32_t c = 0; c < nlist; ++c) {
            const rbq_host::MstgListInfo& L = F.lists[c];
            add(L.off, L.off + L.hdr, 0, gb0[c]);
            const uint64_t nb = (L.n + 31) / 32;
            for (uint64_t j = 0; j < nb; ++j) {
                const uint64_t a = L.off + L.hdr + j * 32 * R, nv = std::min<uint64_t>(32, L.n - j * 32);
                boff[gb0[c] + j] = a; bnv[gb0[c] + j] = (uint32_t)nv;
                add(a, a + nv * R, 1, (uint32_t)(gb0[c] + j));
            }
        }
        if (cur.e > cur.a) spans.push_back(cur);
        for (const Span& s : spans) cap = std::max(cap, s.e - s.a);
    }
    uint64_t* d_boff = nullptr;
    uint32_t *d_bnv = nullptr, *d_seg = nullptr, *d_crcs = nullptr, *d_err = nullptr;
    uint8_t *d_span[2] = {nullptr, nullptr}, *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2];
    HIP_TRY(t.make_stream());
    HIP_TRY(t.alloc(&d_boff, nblocks * 8));
    HIP_TRY(t.alloc(&d_bnv, nblocks * 4));
    HIP_TRY(t.alloc(&d_seg, crc_scratch_words(cap) * 4));
    HIP_TRY(t.alloc(&d_crcs, spans.size() * 4));
    HIP_TRY(t.alloc(&d_err, 4));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(t.alloc(&d_span[i], cap));
        HIP_TRY(t.alloc_pinned(&pin[i], cap));
        HIP_TRY(t.event(&ev[i]));
    }
    HIP_TRY(hipMemcpyAsync(d_boff, boff.data(), nblocks * 8, hipMemcpyHostToDevice, t.stream));
    HIP_TRY(hipMemcpyAsync(d_bnv, bnv.data(), nblocks * 4, hipMemcpyHostToDevice, t.stream));
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, t.stream));
    HIP_TRY(hipStreamSynchronize(t.stream)); // (boff / bnv are host vectors: their copies are done before anything else is queued)

    MstgLoadParams P;
    P.boff = d_boff; P.block_nv = d_bnv; P.blocks = (uint8_t*)ix->blocks.p; P.ids = (uint64_t*)ix->ids.p; P.ex = (uint8_t*)ix->ex.p;
    P.fadd_ex = (float*)ix->fadd_ex.p; P.fres_ex = (float*)ix->fres_ex.p; P.delta = (float*)ix->delta.p; P.vl = (float*)ix->vl.p;
    P.rnorm = (float*)ix->rnorm.p; P.err = d_err; P.D = D; P.Dc = Dc; P.ex_bits = ex_bits; P.R = (uint32_t)R;
    P.E = rbq_host::mstg_ex_len(D, ex_bits);
    // the host reads span i + 1 into one page-locked buffer while the GPU checksums and scatters span i from the other
    for (size_t k = 0; k < spans.size(); ++k) {
        const Span& s = spans[k];
        const int b = (int)(k & 1);
        if (k >= 2) HIP_TRY(hipEventSynchronize(ev[b]));
        if (read(user, s.a, pin[b], s.e - s.a) != 0) return fail(RBQ_IO, "the reader failed at offset " + std::to_string(s.a));
        HIP_TRY(hipMemcpyAsync(d_span[b], pin[b], s.e - s.a, hipMemcpyHostToDevice, t.stream));
        HIP_TRY(launch_crc32(d_span[b], s.e - s.a, d_seg, d_crcs + k, t.stream));
        P.span = d_span[b]; P.span_off = s.a; P.gb_first = s.gb_first; P.nb = s.nb;
        HIP_TRY(launch_mstg_load_scatter(P, t.stream));
        HIP_TRY(hipEventRecord(ev[b], t.stream));
    }
    std::vector<uint32_t> crcs(spans.size());
    uint32_t err = 0, stored = 0;
    HIP_TRY(hipMemcpyAsync(crcs.data(), d_crcs, crcs.size() * 4, hipMemcpyDeviceToHost, t.stream));
    HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, t.stream));
    HIP_TRY(hipStreamSynchronize(t.stream));
    if (err) return fail(RBQ_INVALID_PERSISTENCE, rbq_host::mstg_record_error(err));
    uint32_t crc = F.head_crc;
    for (size_t k = 0; k < spans.size(); ++k) crc = rbq_host::crc32_combine(crc, crcs[k], spans[k].e - spans[k].a);
    if (read(user, F.crc_off, &stored, 4) != 0) return fail(RBQ_IO, "the reader failed at the checksum");
    if (crc != stored) return fail(RBQ_INVALID_PERSISTENCE, "checksum mismatch");

    HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, d_bnv, (uint32_t)nblocks, Dc, (BlockSummary*)ix->bsum.p, 0));
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = finish_replica(ix, ln))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (cfg_out) *cfg_out = F.cfg;
    return wrap_and_replicate(own.release(), devs, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_mstg_save_stream(const rbq_index* idx, const rbq_mstg_config* cfg, rbq_write_fn write, void* user) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return mstg_save_impl(idx, cfg, write, user);
    RBQ_GUARD_END
}

int rbq_mstg_save(const rbq_index* idx, const rbq_mstg_config* cfg, uint8_t** bytes, uint64_t* len) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!bytes || !len) return fail(RBQ_INVALID_CONFIG, "null output");
    *bytes = nullptr; *len = 0;
    int rc = mstg_save_check(idx, cfg);
    if (rc) return rc;
    std::vector<uint64_t> loff;
    mstg_layout(idx->reps[0], loff);
    const uint64_t total = mstg_head_bytes(idx->reps[0]) + loff.back() + 4;
    BufSink sink{(uint8_t*)std::malloc(total), total, 0};
    if (!sink.p) return fail(RBQ_IO, "out of host memory");
    rc = mstg_save_impl(idx, cfg, buf_sink, &sink);
    if (rc == RBQ_OK && sink.len != total) rc = fail(RBQ_IO, "internal error: stream length");
    if (rc) { std::free(sink.p); return rc; }
    *bytes = sink.p; *len = total;
    return RBQ_OK;
    RBQ_GUARD_END
}

int rbq_mstg_load_stream(rbq_read_fn read, void* user, uint64_t total_len, int device, rbq_mstg_config* cfg_out, rbq_index** idx_out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return mstg_load_impl(read, user, total_len, device, cfg_out, idx_out);
    RBQ_GUARD_END
}

int rbq_mstg_load(const void* bytes, uint64_t len, int device, rbq_mstg_config* cfg_out, rbq_index** idx_out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!bytes && len) return fail(RBQ_INVALID_CONFIG, "null buffer");
    MemSrc m{(const uint8_t*)bytes, len};
    return mstg_load_impl(mem_read, &m, len, device, cfg_out, idx_out);
    RBQ_GUARD_END
}

uint64_t rbq_mstg_memory_usage(const rbq_index* idx) {
    if (!idx || idx->reps.empty()) return 0;
    const Replica* ix = idx->reps[0];
    uint64_t total = 0;
    for (const Arr* a : ix->arrays)
        if (a->p && !(a == &ix->raw && ix->raw_borrowed)) total += a->bytes;
    return total;
}
} // extern "C"
