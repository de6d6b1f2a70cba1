// rbq_mstg_file.hpp — the host side of the `.mstg` format (include/rbq_mstg_persist.h; MstgIndex::save_main_index /
// load_main_index, reference src/mstg/io.rs:129-245): section and record lengths, the config and list-header encoders and
// decoders, and the validation of the framing.  Pure C++ (no HIP): librbq.so's api_mstg_persist.hip uses it, and the CPU
// builder exports rbq_build_mstg_file_check over it, which the host tests and the sanitizer build reach.
//
// Framing = everything but the records: magic, version, config, centroid ids, and of every posting list its length prefix
// and header (cluster_id, centroid, size, RabitqConfig, vectors.len()).  The records themselves are validated where they are
// taken apart: by k_mstg_load_scatter on the device, and by mstg_record_flags here for the CPU check.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../../include/rbq_mstg_persist.h"
#include "rbq_host_logic.hpp"

namespace rbq_host {

constexpr uint64_t kMstgCfgBytes = 77;

// what a record can get wrong (k_mstg_load_scatter ORs these into its error word; mstg_record_flags returns them)
enum : uint32_t {
    kMstgBadCodeLen = 1u,    // code.len() != dim of the list
    kMstgBadBinLen = 2u,     // binary_code_packed.len() != dim / 8
    kMstgBadExLen = 4u,      // ex_code_packed.len() != dim / 16 * {2, 4, 12}
    kMstgBadExBits = 8u,     // ex_bits != the list's total_bits - 1
    kMstgBadDim = 16u,       // dim != the centroid's length
    kMstgBadCode = 32u,      // code[i] != ex_code[i] + (bit[i] << ex_bits)
    kMstgBadOneBit = 64u,    // 1-bit: ex_code_packed, f_add_ex or f_rescale_ex is not all zero bits
};
inline std::string mstg_record_error(uint32_t flags) {
    std::string s = "a record disagrees with its list:";
    if (flags & kMstgBadCodeLen) s += " code length;";
    if (flags & kMstgBadBinLen) s += " binary_code_packed length;";
    if (flags & kMstgBadExLen) s += " ex_code_packed length;";
    if (flags & kMstgBadExBits) s += " ex_bits;";
    if (flags & kMstgBadDim) s += " dim;";
    if (flags & kMstgBadCode) s += " code is not ex_code + (bit << ex_bits);";
    if (flags & kMstgBadOneBit) s += " 1-bit record with ex code bytes or extended factors that are not zero;";
    s.pop_back();
    return s;
}

inline uint32_t mstg_ex_len(uint32_t D, uint32_t ex_bits) { return D / 16 * (ex_bits == 0 ? 2u : ex_bits == 2 ? 4u : 12u); }
// one {vector_id, QuantizedVector}: id 8 | code 8 + 2D | binary 8 + D/8 | ex 8 + E | ex_bits 1 | dim 8 | eight f32
inline uint64_t mstg_record_len(uint32_t D, uint32_t ex_bits) { return 73ull + 2ull * D + D / 8 + mstg_ex_len(D, ex_bits); }
// a PostingList before its records: cluster_id 4 | centroid 8 + 4D | size 4 | total_bits 8 | tag 1 (+ 4) | vectors.len() 8
inline uint64_t mstg_list_header_len(uint32_t D, bool has_t) { return 33ull + 4ull * D + (has_t ? 4u : 0u); }
// offsets inside a record
inline uint32_t mstg_rec_off_bin(uint32_t D) { return 16u + 2u * D; }             // the u64 length of binary_code_packed
inline uint32_t mstg_rec_off_ex(uint32_t D) { return mstg_rec_off_bin(D) + 8u + D / 8; } // the u64 length of ex_code_packed
inline uint32_t mstg_rec_off_tail(uint32_t D, uint32_t ex_bits) { return mstg_rec_off_ex(D) + 8u + mstg_ex_len(D, ex_bits); } // ex_bits u8

struct MstgPut {
    uint8_t* o;
    void raw(const void* p, size_t n) { std::memcpy(o, p, n); o += n; }
    void u8(uint8_t v) { *o++ = v; }
    void u32(uint32_t v) { raw(&v, 4); }
    void u64(uint64_t v) { raw(&v, 8); }
    void f32(float v) { raw(&v, 4); }
};

inline void mstg_put_config(const rbq_mstg_config& c, uint8_t out[kMstgCfgBytes]) {
    MstgPut p{out};
    p.u64(c.max_posting_size); p.u64(c.branching_factor); p.f32(c.balance_weight); p.f32(c.closure_epsilon);
    p.u64(c.max_replicas); p.u64(c.rabitq_bits); p.u8(c.faster_config); p.u32(c.metric);
    p.u64(c.hnsw_m); p.u64(c.hnsw_ef_construction); p.u32(c.centroid_precision); p.u64(c.default_ef_search);
    p.f32(c.pruning_epsilon);
}
// null, or what bincode (or this library) refuses in the config
inline const char* mstg_config_error(const rbq_mstg_config& c) {
    if (c.faster_config > 1) return "config: faster_config is not a bool";
    if (c.metric > 1) return "config: unknown metric variant";
    if (c.centroid_precision > 3) return "config: unknown centroid_precision variant";
    if (c.rabitq_bits != 1 && c.rabitq_bits != 3 && c.rabitq_bits != 7)
        return "config: rabitq_bits must be 1, 3 or 7 (ex_bits 0, 2 or 6)";
    return nullptr;
}
inline void mstg_get_config(const uint8_t in[kMstgCfgBytes], rbq_mstg_config& c) {
    const uint8_t* p = in;
    auto get = [&](void* d, size_t n) { std::memcpy(d, p, n); p += n; };
    std::memset(&c, 0, sizeof c);
    get(&c.max_posting_size, 8); get(&c.branching_factor, 8); get(&c.balance_weight, 4); get(&c.closure_epsilon, 4);
    get(&c.max_replicas, 8); get(&c.rabitq_bits, 8); get(&c.faster_config, 1); get(&c.metric, 4);
    get(&c.hnsw_m, 8); get(&c.hnsw_ef_construction, 8); get(&c.centroid_precision, 4); get(&c.default_ef_search, 8);
    get(&c.pruning_epsilon, 4);
}

// the RabitqConfig a list of n vectors carries in an index of (total_bits, has_t, t): an empty list keeps the default
inline void mstg_list_config(uint64_t n, uint32_t total_bits, bool has_t, uint64_t* tb, bool* tag) {
    *tb = n ? total_bits : 7u;
    *tag = n ? has_t : false;
}
// u64 len | header of list c (n vectors of an index of (D, ex_bits, has_t, t)) into o; returns the bytes written
inline size_t mstg_put_list_header(uint8_t* o, uint32_t c, const float* centroid, uint32_t D, uint64_t n, uint32_t ex_bits, bool has_t,
                                   float t) {
    uint64_t tb; bool tag;
    mstg_list_config(n, ex_bits + 1, has_t, &tb, &tag);
    MstgPut p{o};
    p.u64(mstg_list_header_len(D, tag) + n * mstg_record_len(D, ex_bits));
    p.u32(c); p.u64(D); p.raw(centroid, (size_t)D * 4); p.u32((uint32_t)n); p.u64(tb); p.u8(tag ? 1 : 0);
    if (tag) p.f32(t);
    p.u64(n);
    return (size_t)(p.o - o);
}

struct MstgListInfo {
    uint64_t off = 0; // of the list's u64 length prefix in the stream
    uint32_t hdr = 0; // bytes from there to the first record (8 + header)
    uint64_t n = 0;   // records
};
struct MstgFraming {
    rbq_mstg_config cfg;
    uint32_t D = 0, ex_bits = 0;
    bool has_t = false;
    float t_const = 0.0f;
    uint64_t sec_begin = 0;       // first byte of the posting lists (the first list's length prefix)
    uint64_t crc_off = 0;         // the stored checksum: the lists end here
    uint32_t head_crc = 0;        // CRC-32 of [8, sec_begin)
    uint64_t n_vectors = 0;
    std::vector<MstgListInfo> lists;
    std::vector<float> centroids; // [k][D]
};

// Reads and validates the framing of a stream of `total` bytes through rd(offset, dst, n) -> bool (false: unreadable).  Never
// asks for a byte at or beyond `total`.  RBQ_OK, or RBQ_INVALID_PERSISTENCE with *detail.
template <class ReadAt>
int mstg_parse_framing(ReadAt&& rd, uint64_t total, MstgFraming& F, std::string& detail) {
    auto bad = [&](const std::string& m) { detail = m; return (int)RBQ_INVALID_PERSISTENCE; };
    uint64_t off = 0;
    bool short_read = false;
    auto take = [&](void* dst, uint64_t n) {
        if (n > total || off > total - n) { short_read = true; return false; }
        if (!rd(off, dst, n)) { short_read = true; return false; }
        off += n;
        return true;
    };
    const char* trunc = "the stream ends early (truncated, or a length field runs past it)";
    uint8_t head[8];
    if (!take(head, 8)) return bad(trunc);
    if (std::memcmp(head, "MSTG", 4) != 0) return bad("invalid magic bytes");
    uint32_t version;
    std::memcpy(&version, head + 4, 4);
    if (version != 1) return bad("unsupported version");
    if (total < 12) return bad(trunc);
    const uint64_t end = total - 4; // everything hashed lies before the checksum
    uint32_t crc = 0;
    uint64_t cfg_len;
    if (!take(&cfg_len, 8)) return bad(trunc);
    crc = crc32_update(crc, (const uint8_t*)&cfg_len, 8);
    if (cfg_len != kMstgCfgBytes) return bad(cfg_len > end - off ? trunc : "the config block is not the 77 bytes of MstgConfig");
    uint8_t cb[kMstgCfgBytes];
    if (!take(cb, kMstgCfgBytes)) return bad(trunc);
    crc = crc32_update(crc, cb, kMstgCfgBytes);
    mstg_get_config(cb, F.cfg);
    if (const char* why = mstg_config_error(F.cfg)) return bad(why);
    F.ex_bits = (uint32_t)F.cfg.rabitq_bits - 1;
    uint64_t k;
    if (!take(&k, 8)) return bad(trunc);
    crc = crc32_update(crc, (const uint8_t*)&k, 8);
    if (off > end || k > (end - off) / 4) return bad(trunc);
    {
        std::vector<uint32_t> ids((size_t)k);
        if (k && !take(ids.data(), k * 4)) return bad(trunc);
        crc = crc32_update(crc, (const uint8_t*)ids.data(), (size_t)k * 4);
        for (uint64_t i = 0; i < k; ++i)
            if (ids[i] != i) return bad("centroid ids are not 0..k-1 in order");
    }
    uint64_t k2;
    if (!take(&k2, 8)) return bad(trunc);
    crc = crc32_update(crc, (const uint8_t*)&k2, 8);
    if (k2 != k) return bad("the numbers of centroid ids and of posting lists differ");
    if (k == 0) return bad("the index holds no posting list");
    if (off > end || k > (end - off) / (8 + mstg_list_header_len(16, false))) return bad(trunc);
    F.head_crc = crc;
    F.sec_begin = off;
    F.lists.assign((size_t)k, MstgListInfo());
    bool seen = false; // a non-empty list has fixed (has_t, t_const)
    uint64_t nblocks = 0;
    for (uint64_t c = 0; c < k; ++c) {
        MstgListInfo& L = F.lists[c];
        L.off = off;
        uint64_t len, clen;
        uint32_t cid;
        if (!take(&len, 8)) return bad(trunc);
        if (off > end || len > end - off) return bad(trunc);
        const uint64_t body = off;
        if (len < 12) return bad("a posting list is shorter than its header");
        if (!take(&cid, 4) || !take(&clen, 8)) return bad(trunc);
        if (cid != c) return bad("cluster ids are not 0..k-1 in order");
        if (c == 0) {
            if (clen == 0 || clen > 2048 || clen % 16 != 0)
                return bad("dimension (the centroid length) must be a multiple of 16 in 16..2048");
            F.D = (uint32_t)clen;
            F.centroids.resize((size_t)k * F.D);
        } else if (clen != F.D) {
            return bad("the centroids' lengths differ");
        }
        const uint32_t D = F.D;
        if (len < mstg_list_header_len(D, false)) return bad("a posting list is shorter than its header");
        if (!take(&F.centroids[(size_t)c * D], (uint64_t)D * 4)) return bad(trunc);
        uint32_t size;
        uint64_t tb, nvec;
        uint8_t tag;
        float t = 0.0f;
        if (!take(&size, 4) || !take(&tb, 8) || !take(&tag, 1)) return bad(trunc);
        if (tag > 1) return bad("t_const: the Option tag is neither 0 nor 1");
        if (tag && len < mstg_list_header_len(D, true)) return bad("a posting list is shorter than its header");
        if (tag && !take(&t, 4)) return bad(trunc);
        if (!take(&nvec, 8)) return bad(trunc);
        if (size != nvec) return bad("size differs from vectors.len()");
        const uint64_t R = mstg_record_len(D, F.ex_bits), rest = len - (off - body);
        if (nvec > rest / R || nvec * R != rest) return bad("a posting list's length is not its header plus its records");
        if (nvec) {
            if (tb != F.cfg.rabitq_bits) return bad("a posting list's total_bits differs from the config's rabitq_bits");
            uint32_t tbits, fbits;
            std::memcpy(&tbits, &t, 4); std::memcpy(&fbits, &F.t_const, 4);
            if (seen && (F.has_t != (tag != 0) || tbits != fbits)) return bad("the posting lists' t_const differ");
            seen = true; F.has_t = tag != 0; F.t_const = t;
        } else if (tb != 7 || tag) {
            return bad("an empty posting list does not carry RabitqConfig::default() (7, None)");
        }
        L.hdr = (uint32_t)(off - L.off);
        L.n = nvec;
        F.n_vectors += nvec;
        nblocks += (nvec + 31) / 32;
        if (nblocks * 32 > 0xffffffffull) return bad("index too large for 32-bit vector slots");
        off += nvec * R; // the records: not read here
    }
    if (off != end) return bad(off < end ? "bytes between the last posting list and the checksum" : trunc);
    if (F.n_vectors == 0) return bad("the index holds no vector");
    F.crc_off = end;
    (void)short_read;
    return RBQ_OK;
}

// inner fields of one record of a list of (D, ex_bits): 0, or kMstgBad* flags (the CPU statement of the device's checks)
inline uint32_t mstg_record_flags(const uint8_t* r, uint32_t D, uint32_t ex_bits) {
    uint32_t f = 0;
    auto u64at = [&](uint32_t o) { uint64_t v; std::memcpy(&v, r + o, 8); return v; };
    const uint32_t ob = mstg_rec_off_bin(D), oe = mstg_rec_off_ex(D), ot = mstg_rec_off_tail(D, ex_bits), E = mstg_ex_len(D, ex_bits);
    if (u64at(8) != D) f |= kMstgBadCodeLen;
    if (u64at(ob) != D / 8) f |= kMstgBadBinLen;
    if (u64at(oe) != E) f |= kMstgBadExLen;
    if (r[ot] != ex_bits) f |= kMstgBadExBits;
    if (u64at(ot + 1) != D) f |= kMstgBadDim;
    if (f) return f; // (the sections below sit where the lengths say)
    const uint8_t *bin = r + ob + 8, *ex = r + oe + 8;
    for (uint32_t i = 0; i < D; ++i) {
        const uint32_t bit = (bin[i >> 3] >> (7 - (i & 7))) & 1u, t = i >> 4, l = i & 15u;
        uint32_t code = 0;
        if (ex_bits == 2) code = (ex[t * 4 + (l & 3u)] >> (2 * (l >> 2))) & 3u;
        else if (ex_bits == 6)
            code = ((ex[t * 12 + (l & 7u)] >> (l < 8 ? 0 : 4)) & 15u) | (((ex[t * 12 + 8 + (l & 3u)] >> (2 * (l >> 2))) & 3u) << 4);
        uint16_t have;
        std::memcpy(&have, r + 16 + 2 * i, 2);
        if (have != code + (bit << ex_bits)) f |= kMstgBadCode;
    }
    if (ex_bits == 0) {
        for (uint32_t i = 0; i < E; ++i) if (ex[i]) f |= kMstgBadOneBit;
        for (uint32_t i = 0; i < 8; ++i) if (r[ot + 9 + 24 + i]) f |= kMstgBadOneBit;
    }
    return f;
}

// The whole check on the CPU: framing, every record, the checksum.  RBQ_OK or RBQ_INVALID_PERSISTENCE with *detail.
inline int mstg_check_bytes(const uint8_t* bytes, uint64_t len, MstgFraming& F, std::string& detail) {
    auto rd = [&](uint64_t off, void* dst, uint64_t n) { std::memcpy(dst, bytes + off, (size_t)n); return true; };
    const int rc = mstg_parse_framing(rd, len, F, detail);
    if (rc) return rc;
    const uint64_t R = mstg_record_len(F.D, F.ex_bits);
    uint32_t flags = 0;
    for (const MstgListInfo& L : F.lists)
        for (uint64_t i = 0; i < L.n; ++i) flags |= mstg_record_flags(bytes + L.off + L.hdr + i * R, F.D, F.ex_bits);
    if (flags) { detail = mstg_record_error(flags); return RBQ_INVALID_PERSISTENCE; }
    uint32_t stored;
    std::memcpy(&stored, bytes + F.crc_off, 4);
    if (crc32_ieee(bytes + 8, (size_t)(F.crc_off - 8)) != stored) { detail = "checksum mismatch"; return RBQ_INVALID_PERSISTENCE; }
    return RBQ_OK;
}

} // namespace rbq_host
