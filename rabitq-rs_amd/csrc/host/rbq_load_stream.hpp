// rbq_load_stream.hpp — the GPU-free half of rbq_index_load_rbq1_stream (include/rbq_persist.h): the framing pass over a
// reader, the span cutter with its piece descriptors, the ex-code prefix check as a plain loop, and the verdict.  Pure C++
// (no HIP): librbq.so's api_load.hip includes it, k_load.hip takes LoadPiece from it, and tests/loadcheck_main.cpp runs the
// same code with -fsanitize=address,undefined against rbq1_parse on a machine without a GPU.
//
// A cluster of an RBQ1 stream, in file order (rbq1_parse, rbq_host_logic.hpp):
//   centroid D f32 | n u64 | ids n u64 | blen u64 | batch_data ceil(n/32) x (4D + 384) | n x (u64 len | ex code) |
//   f_add_ex n f32 | f_rescale_ex n f32 | delta n f32 | vl n f32
// so every offset inside it follows from n alone.  The loader's answer for any byte string is rbq1_parse's: the first
// failing check in file order.  The framing pass finds every failure that needs no record bytes and remembers the first;
// the only check it cannot make is an ex code's length prefix, so the record pass looks at every prefix that lies BEFORE
// the remembered failure (region_end below) and a wrong one there wins.
#pragma once
#include "rbq_host_logic.hpp"

namespace rbq_host {

// sections of a cluster in file order; the value is LoadPiece::kind
enum : uint32_t { kLpCentroid = 0, kLpN, kLpIds, kLpBlen, kLpBatch, kLpEx, kLpFadd, kLpFres, kLpDelta, kLpVl, kLpSections };

// One run of whole units of one section of one list inside a span.  `first` is where its first unit goes in the device
// layout: centroid: f32 index c * D + i; batch: global block; ids, ex, factors: global slot.  `fill`: pad slots behind the
// list's last vector (this piece holds it) that get the fill value.  wg0: first workgroup of the piece in the span's launch.
struct LoadPiece {
    uint64_t off;   // byte offset of the first unit in the span
    uint64_t first;
    uint32_t count; // units
    uint32_t fill;
    uint32_t kind;
    uint32_t wg0;
};

constexpr uint64_t kLoadSpanDefault = 64ull << 20, kLoadSpanMax = 1ull << 30;
constexpr uint32_t kLoadMaxPieces = 1u << 16; // a span closes at this many pieces (the piece tables stay 2 MB)

struct LoadGeom {
    uint64_t D = 0, stride = 0, exb = 0; // padded_dim, bytes of a batch record, bytes of a packed ex code
    uint64_t unit(uint32_t kind) const {
        switch (kind) {
            case kLpCentroid: case kLpFadd: case kLpFres: case kLpDelta: case kLpVl: return 4;
            case kLpBatch: return stride;
            case kLpEx: return 8 + exb;
            default: return 8;
        }
    }
    uint64_t units(uint32_t kind, uint64_t n) const {
        switch (kind) {
            case kLpCentroid: return D;
            case kLpN: case kLpBlen: return 1;
            case kLpBatch: return (n + 31) / 32;
            default: return n;
        }
    }
    uint64_t cluster_bytes(uint64_t n) const { return D * 4 + 16 + n * 8 + (n + 31) / 32 * stride + n * (8 + exb) + n * 16; }
};

struct LoadFraming {
    rbq_header h;                   // (rotator_blob stays null: the caller reads the blob at rot_off)
    LoadGeom g;
    uint64_t rot_off = 0;           // the rotator blob: [rot_off, cluster_begin)
    uint64_t cluster_begin = 0;     // first byte of the cluster region
    std::vector<uint64_t> list_off; // file offset of every framed cluster; the last one may be cut short by region_end
    std::vector<uint32_t> list_n;
    uint64_t region_end = 0;        // the record pass covers the whole units of [cluster_begin, region_end)
    uint64_t body_end = 0;          // no failure: where the stored CRC lies
    uint64_t actual = 0;            // vectors of the framed clusters
    int fail_rc = RBQ_OK;           // the first failing check that needs no record bytes
    std::string fail_detail;
    bool header_ok = false;         // the header and rotator length passed: h, g, rot_off and cluster_begin are valid
    bool complete() const { return fail_rc == RBQ_OK; }
};

inline bool load_fits(uint64_t off, uint64_t n, uint64_t total) { return n <= total && off <= total - n; }

// The framing pass.  rd(off, dst, n) -> bool reads n bytes inside [0, total).  Returns false when rd failed (the caller
// reports RBQ_IO "read callback failed"); every other outcome is in F.
template <class Rd>
bool load_frame(Rd&& rd, uint64_t total, LoadFraming& F) {
    auto fail = [&](int code, const char* msg) { F.fail_rc = code; F.fail_detail = msg; return true; };
    auto eof = [&] { return fail(RBQ_IO, "failed to fill whole buffer"); };
    std::memset(&F.h, 0, sizeof F.h);
    uint8_t head[44];
    const size_t hl = (size_t)std::min<uint64_t>(44, total);
    if (hl && !rd(0, head, hl)) return false;
    Reader r{head, hl};
    // (the header checks are rbq1_parse's, statement for statement)
    char magic[4];
    if (!r.take(magic, 4)) return eof();
    if (std::memcmp(magic, "RBQ1", 4) != 0) return fail(RBQ_INVALID_PERSISTENCE, "unrecognized file header");
    uint32_t version;
    if (!r.take(&version, 4)) return eof();
    if (version != 3) return fail(RBQ_INVALID_PERSISTENCE, "unsupported index format version (expected V3 with unified memory layout)");
    rbq_header& h = F.h;
    uint8_t tags[4];
    if (!r.take(&h.dim, 4)) return eof();
    if (h.dim == 0) return fail(RBQ_INVALID_PERSISTENCE, "dimension must be positive");
    if (!r.take(&h.padded_dim, 4)) return eof();
    if (h.padded_dim < h.dim) return fail(RBQ_INVALID_PERSISTENCE, "padded_dim must be >= dim");
    if (!r.take(tags, 4)) return eof();
    if (tags[0] > 1) return fail(RBQ_INVALID_PERSISTENCE, "unknown metric tag");
    if (tags[1] > 1) return fail(RBQ_INVALID_PERSISTENCE, "unknown rotator type tag");
    if (tags[2] > 16) return fail(RBQ_INVALID_PERSISTENCE, "ex_bits out of range");
    if (tags[3] == 0 || tags[3] > 16) return fail(RBQ_INVALID_PERSISTENCE, "total_bits out of range");
    if ((uint8_t)(tags[3] - 1) != tags[2]) return fail(RBQ_INVALID_PERSISTENCE, "total_bits does not match ex_bits");
    h.metric = tags[0]; h.rotator = tags[1]; h.ex_bits = tags[2];
    uint64_t expected_vectors, cluster_count, rot_len;
    if (!r.take(&expected_vectors, 8) || !r.take(&cluster_count, 8) || !r.take(&rot_len, 8)) return eof();
    if (!load_fits(44, rot_len, total)) return eof();
    h.rotator_len = rot_len; h.n_lists = cluster_count; h.n_vectors = expected_vectors;
    {
        const uint64_t want = h.rotator == RBQ_ROTATOR_FHT_KAC ? (uint64_t)4 * h.padded_dim / 8 : (uint64_t)h.padded_dim * h.padded_dim * 4;
        if (rot_len != want)
            return fail(RBQ_INVALID_PERSISTENCE, h.rotator == RBQ_ROTATOR_FHT_KAC ? "FHT rotator flip bits length mismatch" : "rotator matrix length mismatch");
    }
    F.rot_off = 44; F.cluster_begin = 44 + rot_len; F.region_end = F.cluster_begin;
    F.g.D = h.padded_dim; F.g.stride = F.g.D * 4 + 384; F.g.exb = h.ex_bits ? F.g.D * h.ex_bits / 8 : 0;
    F.header_ok = true;
    if (cluster_count > total / 8) return eof();
    const LoadGeom& g = F.g;
    uint64_t off = F.cluster_begin;
    for (uint64_t c = 0; c < cluster_count; ++c) {
        // a cluster that ends early is framed as far as its n is known: the prefixes it still holds come before the end
        const uint64_t c0 = off;
        if (!load_fits(off, g.D * 4, total)) return eof();
        off += g.D * 4;
        uint64_t n;
        if (!load_fits(off, 8, total)) return eof();
        if (!rd(off, &n, 8)) return false;
        off += 8;
        if (n > 1000000) return fail(RBQ_INVALID_PERSISTENCE, "cluster size exceeds reasonable limits - possible corruption");
        const uint64_t o_blen = off + n * 8, nb = (n + 31) / 32;
        if (!load_fits(off, n * 8, total) || !load_fits(o_blen, 8, total)) return eof();
        uint64_t blen;
        if (!rd(o_blen, &blen, 8)) return false;
        if (blen != nb * g.stride)
            return fail(RBQ_INVALID_PERSISTENCE, "batch_data length mismatch - possible corruption or version incompatibility");
        F.list_off.push_back(c0);
        F.list_n.push_back((uint32_t)n);
        const uint64_t end = c0 + g.cluster_bytes(n);
        if (!load_fits(c0, g.cluster_bytes(n), total)) {
            F.region_end = total;
            // the stream ends inside an ex code whose prefix is whole: rbq1_parse checks that prefix before it runs out of
            // bytes, and the record pass sees whole records only
            const uint64_t ex0 = o_blen + 8 + nb * g.stride, rec = 8 + g.exb;
            if (total > ex0 && total < ex0 + n * rec) {
                const uint64_t p = ex0 + (total - ex0) / rec * rec;
                uint64_t el;
                if (total - p >= 8) {
                    if (!rd(p, &el, 8)) return false;
                    if (el != g.exb)
                        return fail(RBQ_INVALID_PERSISTENCE, "ex_code_packed length mismatch - possible corruption or version incompatibility");
                }
            }
            return eof();
        }
        F.actual += n;
        off = end;
        F.region_end = end;
    }
    F.body_end = off;
    return true;
}

// Cuts the cluster region into spans and their pieces.  next() fills `pieces` with the pieces of the next span (file bytes
// [*span_off, *span_off + *span_len), at most `budget` bytes and kLoadMaxPieces pieces) and returns false when the region is
// exhausted.  budget >= the largest unit (load_span_budget).  Pieces follow each other without gaps inside a span, spans
// without gaps inside the region.
inline uint64_t load_span_budget(uint64_t requested, const LoadGeom& g) {
    uint64_t b = requested ? requested : kLoadSpanDefault;
    b = std::min(b, kLoadSpanMax);
    return std::max(b, std::max(g.stride, 8 + g.exb));
}

struct LoadCutter {
    const LoadFraming& F;
    uint64_t budget;
    uint64_t c = 0, u = 0, pos, gb = 0; // cluster, unit inside the section, file offset, first block of cluster c
    uint32_t sec = 0;
    bool done = false;
    LoadCutter(const LoadFraming& f, uint64_t budget_) : F(f), budget(budget_), pos(f.cluster_begin) {}
    bool next(std::vector<LoadPiece>& pieces, uint64_t* span_off, uint64_t* span_len) {
        pieces.clear();
        const LoadGeom& g = F.g;
        const uint64_t a = pos;
        while (!done && c < F.list_n.size() && pieces.size() < kLoadMaxPieces) {
            const uint64_t n = F.list_n[c], us = g.unit(sec), left = g.units(sec, n) - u;
            if (!left) {
                u = 0;
                if (++sec == kLpSections) { sec = 0; gb += (n + 31) / 32; ++c; }
                continue;
            }
            const uint64_t room_region = (F.region_end - pos) / us;
            if (!room_region) { done = true; break; } // the region ends inside this section (a stream cut short)
            const uint64_t take = std::min(left, std::min(room_region, (budget - (pos - a)) / us));
            if (!take) break; // the span is full
            LoadPiece p;
            p.off = pos - a; p.count = (uint32_t)take; p.kind = sec; p.fill = 0; p.wg0 = 0;
            if (sec == kLpCentroid) p.first = c * g.D + u;
            else if (sec == kLpBatch) p.first = gb + u;
            else p.first = gb * 32 + u;
            if (sec != kLpCentroid && sec != kLpBatch && sec != kLpN && sec != kLpBlen && u + take == n) p.fill = (uint32_t)((32 - n % 32) % 32);
            pieces.push_back(p);
            pos += take * us; u += take;
        }
        *span_off = a; *span_len = pos - a;
        return pos > a;
    }
};

// Workgroups (256 threads) of every piece in the span's scatter launch, in LoadPiece::wg0; returns their number.
// scatter: the index arrays exist and are written; otherwise only the ex-code prefixes are checked.
inline uint64_t load_assign_workgroups(std::vector<LoadPiece>& pieces, uint32_t ex_bits, bool scatter) {
    uint64_t wg = 0;
    for (LoadPiece& p : pieces) {
        p.wg0 = (uint32_t)wg;
        const uint64_t slots = (uint64_t)p.count + p.fill;
        switch (p.kind) {
            case kLpCentroid: if (scatter) wg += ((uint64_t)p.count + 255) / 256; break;
            case kLpIds: case kLpDelta: case kLpVl: if (scatter) wg += (slots + 255) / 256; break;
            case kLpFadd: case kLpFres: if (scatter && ex_bits) wg += (slots + 255) / 256; break;
            case kLpBatch: if (scatter) wg += ((uint64_t)p.count + 7) / 8; break;
            case kLpEx: wg += scatter && ex_bits ? (slots + 15) / 16 : ((uint64_t)p.count + 255) / 256; break;
            default: break;
        }
    }
    return wg;
}

// The GPU's prefix check as a plain loop: the lowest file position of an ex-code length prefix of the span that is not
// g.exb, or ~0 (span: the bytes of the span, which lies at file offset span_off).
inline uint64_t load_check_prefixes(const uint8_t* span, uint64_t span_off, const std::vector<LoadPiece>& pieces, const LoadGeom& g) {
    for (const LoadPiece& p : pieces) {
        if (p.kind != kLpEx) continue;
        for (uint64_t i = 0; i < p.count; ++i) {
            uint64_t el;
            std::memcpy(&el, span + p.off + i * (8 + g.exb), 8);
            if (el != g.exb) return span_off + p.off + i * (8 + g.exb);
        }
    }
    return ~0ull;
}

constexpr uint64_t kLoadNoBadPrefix = ~0ull;

// The verdict, in rbq1_parse's order.  bad_prefix: the lowest offending prefix position of the record pass.  Stage 1 needs
// no CRC; when it returns RBQ_OK with *want_stored set, the caller reads the stored CRC at F.body_end and asks stage 2.
inline int load_verdict_framing(const LoadFraming& F, uint64_t bad_prefix, uint64_t total, std::string* detail, bool* want_stored) {
    auto fail = [&](int code, const std::string& msg) { *detail = msg; return code; };
    *want_stored = false;
    if (bad_prefix != kLoadNoBadPrefix)
        return fail(RBQ_INVALID_PERSISTENCE, "ex_code_packed length mismatch - possible corruption or version incompatibility");
    if (F.fail_rc) return fail(F.fail_rc, F.fail_detail);
    if (F.actual != F.h.n_vectors) return fail(RBQ_INVALID_PERSISTENCE, "vector count metadata mismatch");
    if (!load_fits(F.body_end, 4, total)) return fail(RBQ_IO, "failed to fill whole buffer");
    *want_stored = true;
    return RBQ_OK;
}
inline int load_verdict_crc(uint32_t crc, uint32_t stored, std::string* detail) {
    if (crc != stored) { *detail = "checksum mismatch"; return RBQ_INVALID_PERSISTENCE; }
    return RBQ_OK;
}

} // namespace rbq_host
