// rbq_host_logic.hpp — the host-side logic of the C ABI that touches no GPU: the RBQ1-v3 stream parser / validator
// (load_from_reader, reference src/ivf.rs:1484-1702), CRC-32/IEEE, and the sub-batch / shard / result-packing arithmetic
// of rbq_search_batch.  Pure C++ (no HIP): librbq.so includes it, and tests/test_sanitizers.py builds the same code with
// -fsanitize=address,undefined (csrc/host/rbq_hostcheck.cpp) and fuzzes it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "rbq.h"

namespace rbq_host {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// One ClusterData as byte ranges (an RBQ1 stream has no alignment; rbq_list_view arrays are viewed the same way).
struct ListSrc {
    const uint8_t* centroid = nullptr; // D f32
    uint64_t n = 0;
    const uint8_t* ids = nullptr;        // n u64
    const uint8_t* batch_data = nullptr; // ceil(n/32) records of D*4 + 384 bytes
    const uint8_t* ex = nullptr;         // n packed ex codes, `ex_stride` bytes apart
    size_t ex_stride = 0;
    const uint8_t* fadd = nullptr;       // n f32
    const uint8_t* fres = nullptr;       // n f32
    const uint8_t* delta = nullptr;      // n f32 (reconstruction factors; null: the source has none)
    const uint8_t* vl = nullptr;         // n f32
};

struct Reader {
    const uint8_t* p; size_t len, off = 0;
    bool take(void* dst, size_t n) { if (off + n > len || off + n < off) return false; std::memcpy(dst, p + off, n); off += n; return true; }
    const uint8_t* view(size_t n) { if (off + n > len || off + n < off) return nullptr; const uint8_t* r = p + off; off += n; return r; }
};

// GF(2) arithmetic of CRC-32/IEEE (reflected, polynomial 0xEDB88320), zlib's crc32_combine: with A = crc32(a) and
// B = crc32(b), crc32(a || b) = (A * x^(8 len(b)) mod P) ^ B.  The device CRC (k_save.hip) uses the same formulas.
inline uint32_t crc32_multmodp(uint32_t a, uint32_t b) { // a(x) * b(x) mod P(x), bit 31 = x^0
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
inline uint32_t crc32_x8nmodp(uint64_t n) { // x^(8n) mod P(x)
    uint32_t p = 1u << 31, sq = 1u << 23;   // x^0; x^8
    while (n) {
        if (n & 1) p = crc32_multmodp(sq, p);
        sq = crc32_multmodp(sq, sq);
        n >>= 1;
    }
    return p;
}
inline uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return crc32_multmodp(crc32_x8nmodp(len_b), crc_a) ^ crc_b;
}

inline uint32_t crc32_ieee(const uint8_t* p, size_t n) {
    static uint32_t table[8][256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) table[t][i] = (table[t - 1][i] >> 8) ^ table[0][table[t - 1][i] & 0xff];
    });
    uint32_t crc = ~0u;
    while (n >= 8) {
        uint32_t a, b;
        std::memcpy(&a, p, 4); std::memcpy(&b, p + 4, 4);
        a ^= crc;
        crc = table[7][a & 0xff] ^ table[6][(a >> 8) & 0xff] ^ table[5][(a >> 16) & 0xff] ^ table[4][a >> 24] ^
              table[3][b & 0xff] ^ table[2][(b >> 8) & 0xff] ^ table[1][(b >> 16) & 0xff] ^ table[0][b >> 24];
        p += 8; n -= 8;
    }
    while (n--) crc = table[0][(crc ^ *p++) & 0xff] ^ (crc >> 8);
    return ~crc;
}

// Incremental form: crc32_update(crc32_update(0, a), b) == crc32_ieee(a || b); crc32_update(0, p, n) == crc32_ieee(p, n).
inline uint32_t crc32_update(uint32_t crc, const uint8_t* p, size_t n) {
    if (!n) return crc;
    return crc32_combine(crc, crc32_ieee(p, n), n);
}

// Parses and validates an RBQ1 v3 stream in place (the lists are byte ranges of `bytes`: nothing is copied).  Returns
// RBQ_OK or the error code with the reference's message in *detail — the checks, their order and their strings are
// load_from_reader's (src/ivf.rs:1484-1702; DynamicRotator::deserialize src/rotation.rs:213-219,491-497).  The header's
// rotator_blob points into `bytes`.  What THIS build cannot serve (ex_bits outside {0,2,6}, padded_dim > 2048 ...) is
// left to the caller's validate_header.
inline int rbq1_parse(const void* bytes, size_t len, rbq_header* hout, std::vector<ListSrc>* lists_out, std::string* detail) {
    auto fail = [&](int code, const char* msg) { if (detail) *detail = msg; return code; };
    auto eof = [&] { return fail(RBQ_IO, "failed to fill whole buffer"); };
    if (!bytes) return fail(RBQ_IO, "null buffer");
    Reader r{(const uint8_t*)bytes, len};
    char magic[4];
    if (!r.take(magic, 4)) return eof();
    if (std::memcmp(magic, "RBQ1", 4) != 0) return fail(RBQ_INVALID_PERSISTENCE, "unrecognized file header");
    uint32_t version;
    if (!r.take(&version, 4)) return eof();
    if (version != 3) return fail(RBQ_INVALID_PERSISTENCE, "unsupported index format version (expected V3 with unified memory layout)");
    rbq_header h;
    std::memset(&h, 0, sizeof h);
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
    const uint8_t* blob = r.view(rot_len);
    if (!blob) return eof();
    h.rotator_blob = blob; h.rotator_len = rot_len; h.n_lists = cluster_count; h.n_vectors = expected_vectors;
    { // DynamicRotator::deserialize length checks
        const uint64_t want = h.rotator == RBQ_ROTATOR_FHT_KAC ? (uint64_t)4 * h.padded_dim / 8 : (uint64_t)h.padded_dim * h.padded_dim * 4;
        if (rot_len != want)
            return fail(RBQ_INVALID_PERSISTENCE, h.rotator == RBQ_ROTATOR_FHT_KAC ? "FHT rotator flip bits length mismatch" : "rotator matrix length mismatch");
    }
    if (cluster_count > (len / 8)) return eof(); // every cluster costs >= 8 bytes; guards the allocation below
    const size_t D = h.padded_dim, stride = D * 4 + 384;
    const size_t exb_expected = h.ex_bits ? D * h.ex_bits / 8 : 0;
    std::vector<ListSrc> lists(cluster_count);
    uint64_t actual = 0;
    for (uint64_t c = 0; c < cluster_count; ++c) {
        ListSrc& L = lists[c];
        L.centroid = r.view(D * 4);
        if (!L.centroid) return eof();
        uint64_t n;
        if (!r.take(&n, 8)) return eof();
        if (n > 1000000) return fail(RBQ_INVALID_PERSISTENCE, "cluster size exceeds reasonable limits - possible corruption");
        L.n = n;
        L.ids = r.view(n * 8);
        if (!L.ids) return eof();
        uint64_t blen;
        if (!r.take(&blen, 8)) return eof();
        if (blen != ((n + 31) / 32) * stride)
            return fail(RBQ_INVALID_PERSISTENCE, "batch_data length mismatch - possible corruption or version incompatibility");
        L.batch_data = r.view(blen);
        if (!L.batch_data) return eof();
        L.ex_stride = exb_expected + 8; // every packed code carries a u64 length prefix
        for (uint64_t v = 0; v < n; ++v) {
            uint64_t el;
            if (!r.take(&el, 8)) return eof();
            if (el != exb_expected)
                return fail(RBQ_INVALID_PERSISTENCE, "ex_code_packed length mismatch - possible corruption or version incompatibility");
            const uint8_t* e = r.view(el);
            if (!e) return eof();
            if (v == 0) L.ex = e;
        }
        L.fadd = r.view(n * 4);
        L.fres = r.view(n * 4);
        if (!L.fadd || !L.fres) return eof();
        L.delta = r.view(n * 4); // delta, vl: reconstruction only (kept for rbq_index_save_rbq1)
        L.vl = r.view(n * 4);
        if (!L.delta || !L.vl) return eof();
        actual += n;
    }
    if (actual != expected_vectors) return fail(RBQ_INVALID_PERSISTENCE, "vector count metadata mismatch");
    const size_t body_end = r.off;
    uint32_t stored;
    if (!r.take(&stored, 4)) return eof();
    if (crc32_ieee((const uint8_t*)bytes + 8, body_end - 8) != stored) return fail(RBQ_INVALID_PERSISTENCE, "checksum mismatch");
    *hout = h;
    *lists_out = std::move(lists);
    return RBQ_OK;
}

// ---- RBF1: the persisted form of BruteForceRabitqIndex (reference src/brute_force.rs:305-520) ----------------------------
// One vector's record is  binary_code_packed [ceil(D/8)] | ex_code_packed [ex_len] | delta vl f_add f_rescale f_error
// residual_norm f_add_ex f_rescale_ex (8 x f32 LE); records follow each other with no padding.
struct BfSrc {
    const uint8_t* rec0 = nullptr; // first record
    size_t stride = 0;             // bytes per record
    size_t bin_len = 0, ex_len = 0;
    uint64_t n = 0;
};

// Parses and validates an RBF1 stream in place.  The checks, their order and their strings are load_from_reader's
// (brute_force.rs:395-520; DynamicRotator::deserialize src/rotation.rs:213-219,491-497); truncation is RBQ_IO "failed to fill
// whole buffer", as in rbq1_parse.  The reader expects ceil(D*ex/8) ex-code bytes per vector and none when ex_bits == 0, so
// the 1-bit streams the crate writes (D/8 zero bytes of ex code per vector, see rbf1_write) end in "checksum mismatch" here as
// they do in the crate.  What this build cannot serve (ex_bits outside {0,2,6} ...) is left to the caller.
inline int rbf1_parse(const void* bytes, size_t len, rbq_header* hout, BfSrc* out, std::string* detail) {
    auto fail = [&](int code, const char* msg) { if (detail) *detail = msg; return code; };
    auto eof = [&] { return fail(RBQ_IO, "failed to fill whole buffer"); };
    if (!bytes) return fail(RBQ_IO, "null buffer");
    Reader r{(const uint8_t*)bytes, len};
    char magic[4];
    if (!r.take(magic, 4)) return eof();
    if (std::memcmp(magic, "RBF1", 4) != 0) return fail(RBQ_INVALID_PERSISTENCE, "unrecognized file header");
    uint32_t version;
    if (!r.take(&version, 4)) return eof();
    if (version != 1) return fail(RBQ_INVALID_PERSISTENCE, "unsupported index format version");
    rbq_header h;
    std::memset(&h, 0, sizeof h);
    uint8_t tag;
    if (!r.take(&h.dim, 4)) return eof();
    if (h.dim == 0) return fail(RBQ_INVALID_PERSISTENCE, "dimension must be positive");
    if (!r.take(&h.padded_dim, 4)) return eof();
    if (h.padded_dim < h.dim) return fail(RBQ_INVALID_PERSISTENCE, "padded_dim must be >= dim");
    if (!r.take(&tag, 1)) return eof();
    if (tag > 1) return fail(RBQ_INVALID_PERSISTENCE, "unknown metric tag");
    h.metric = tag;
    if (!r.take(&tag, 1)) return eof();
    if (tag > 1) return fail(RBQ_INVALID_PERSISTENCE, "unknown rotator type tag");
    h.rotator = tag;
    uint8_t ex_bits, total_bits;
    if (!r.take(&ex_bits, 1)) return eof();
    if (ex_bits > 16) return fail(RBQ_INVALID_PERSISTENCE, "ex_bits out of range");
    if (!r.take(&total_bits, 1)) return eof();
    if (total_bits == 0 || total_bits > 16) return fail(RBQ_INVALID_PERSISTENCE, "total_bits out of range");
    if ((uint8_t)(total_bits - 1) != ex_bits) return fail(RBQ_INVALID_PERSISTENCE, "total_bits does not match ex_bits");
    h.ex_bits = ex_bits;
    uint64_t count, rot_len;
    if (!r.take(&count, 8) || !r.take(&rot_len, 8)) return eof();
    const uint8_t* blob = r.view(rot_len);
    if (!blob) return eof();
    h.rotator_blob = blob; h.rotator_len = rot_len; h.n_vectors = count; h.n_lists = 0;
    { // DynamicRotator::deserialize length checks
        const uint64_t want = h.rotator == RBQ_ROTATOR_FHT_KAC ? (uint64_t)4 * h.padded_dim / 8 : (uint64_t)h.padded_dim * h.padded_dim * 4;
        if (rot_len != want)
            return fail(RBQ_INVALID_PERSISTENCE, h.rotator == RBQ_ROTATOR_FHT_KAC ? "FHT rotator flip bits length mismatch" : "rotator matrix length mismatch");
    }
    BfSrc b;
    b.n = count;
    b.bin_len = ((size_t)h.padded_dim + 7) / 8;
    b.ex_len = ex_bits ? ((size_t)h.padded_dim * ex_bits + 7) / 8 : 0;
    b.stride = b.bin_len + b.ex_len + 32;
    if (count > (len - r.off) / b.stride) return eof(); // the records do not fit what is left (also guards the product below)
    b.rec0 = r.view((size_t)count * b.stride);
    if (!b.rec0) return eof();
    const size_t body_end = r.off;
    uint32_t stored;
    if (!r.take(&stored, 4)) return eof();
    if (crc32_ieee((const uint8_t*)bytes + 8, body_end - 8) != stored) return fail(RBQ_INVALID_PERSISTENCE, "checksum mismatch");
    *hout = h;
    *out = b;
    return RBQ_OK;
}

// save_to_writer (brute_force.rs:305-386), byte for byte: header fields, rotator blob, then for every vector its binary code,
// `ex_len` bytes of ex code and the 8 factors, then the CRC-32 of everything after the version field.  `ex_len` is what the
// index holds per vector: ceil(D*ex/8) for ex_bits > 0; for ex_bits == 0 the crate's freshly trained vectors carry
// D/16*2 zero bytes (quantizer.rs:212-219) that it writes and its own reader does not expect, a loaded index carries none.
// bin / ex: [n][bin_len] / [n][ex_len] (ex may be null when ex_len == 0 or for zeros); f[8]: the 8 factor arrays [n].
inline std::vector<uint8_t> rbf1_write(const rbq_header& h, uint64_t n, const uint8_t* bin, const uint8_t* ex, size_t ex_len,
                                       const float* const f[8]) {
    const size_t bin_len = ((size_t)h.padded_dim + 7) / 8, stride = bin_len + ex_len + 32;
    std::vector<uint8_t> o;
    o.reserve(8 + 4 + 4 + 4 + 16 + h.rotator_len + (size_t)n * stride + 4);
    auto put = [&](const void* p, size_t k) { const uint8_t* c = (const uint8_t*)p; o.insert(o.end(), c, c + k); };
    put("RBF1", 4);
    const uint32_t version = 1;
    put(&version, 4);
    put(&h.dim, 4);
    put(&h.padded_dim, 4);
    const uint8_t tags[4] = {h.metric, h.rotator, h.ex_bits, (uint8_t)(h.ex_bits + 1)};
    put(tags, 4);
    put(&n, 8);
    put(&h.rotator_len, 8);
    if (h.rotator_len) put(h.rotator_blob, h.rotator_len);
    const std::vector<uint8_t> zeros(ex_len, 0);
    for (uint64_t v = 0; v < n; ++v) {
        put(bin + v * bin_len, bin_len);
        put(ex ? ex + v * ex_len : zeros.data(), ex_len);
        for (int k = 0; k < 8; ++k) put(&f[k][v], 4);
    }
    const uint32_t crc = crc32_ieee(o.data() + 8, o.size() - 8);
    put(&crc, 4);
    return o;
}

// layout of one sub-batch's results in the packed device / pinned buffers
struct OutPack {
    size_t o_ids, o_scores, o_counts, o_diag, total;
    OutPack(uint64_t n, uint32_t top_k, bool diag) {
        o_ids = 0; o_scores = align_up(n * top_k * 8, 16); o_counts = o_scores + align_up(n * top_k * 4, 16);
        o_diag = o_counts + align_up(n * 4, 16); total = o_diag + (diag ? n * sizeof(rbq_diag) : 0);
    }
};

// The query rows of a search call as the entry points take them (option "query_dtype": RBQ_RAW_F32, or RBQ_RAW_F16 / RBQ_RAW_BF16 —
// rows of `dim` 16-bit elements, 2 * dim bytes apart, behind the `const float*` parameter).  THE copy of the byte arithmetic on
// query rows: lengths of copies and staging buffers, and the first byte of query q (of a sub-batch, a shard, a chunk).
struct QueryRows {
    int dtype = RBQ_RAW_F32;
    uint32_t dim = 0;
    size_t elem_bytes() const { return dtype == RBQ_RAW_F32 ? 4 : 2; }
    size_t row_bytes() const { return (size_t)dim * elem_bytes(); }
    size_t bytes(uint64_t n) const { return (size_t)n * row_bytes(); } // n whole rows
    const float* at(const float* base, uint64_t q) const { return (const float*)((const uint8_t*)base + bytes(q)); } // row q
    // whether `p` may hold such rows: 16-bit rows need a 2-byte aligned base (f32 rows: as ever, not looked at)
    bool aligned(const void* p) const { return dtype == RBQ_RAW_F32 || ((uintptr_t)p & 1u) == 0; }
};

// replica r of R serves the contiguous query shard [q0, q1) of a batch of nq (batch_search is a par_iter over queries)
inline void shard_range(uint64_t r, uint64_t R, uint64_t nq, uint64_t* q0, uint64_t* q1) { *q0 = r * nq / R; *q1 = (r + 1) * nq / R; }

// Sub-batches of one rbq_search_batch call (or replica shard) of nq queries, as (first query, count) in order.
//   nq < 256            one sub-batch
//   nq <= 2048          four sub-batches in the proportion 4:3:2:1 (multiples of 32 queries) over four lanes: the large ones
//                       go first and run under the preparation of the later ones, the last one — whose kernel chain the caller
//                       waits for — is small.  (Round 4, GIST-1M shape, page-locked buffers: 2048 queries per call 532 -> 462 us
//                       against equal quarters, 562 against halves; 1024 per call: 296 either way — such a call is the time the
//                       GPU needs for 1024 queries at its pipelined rate plus the latency of one four-kernel chain.)
//   above               sub-batches of 1024 (which also bounds the nq x n_lists score matrix per lane); a tapered tail was
//                       measured slower there (4096 per call: 828 against 688 us — the chip is saturated, smaller kernels only
//                       add launches)
// `forced` (diagnostic option host_subbatch) gives equal sub-batches of that size.
inline std::vector<std::pair<uint64_t, uint64_t>> subbatch_plan(uint64_t nq, uint64_t forced) {
    std::vector<std::pair<uint64_t, uint64_t>> plan;
    if (nq == 0) return plan;
    if (forced) {
        for (uint64_t q0 = 0; q0 < nq; q0 += forced) plan.emplace_back(q0, std::min<uint64_t>(forced, nq - q0));
        return plan;
    }
    auto taper = [&](uint64_t q0, uint64_t n, std::initializer_list<uint64_t> weights) {
        uint64_t wsum = 0;
        for (uint64_t w : weights) wsum += w;
        uint64_t left = n, pos = q0;
        size_t i = 0;
        for (uint64_t w : weights) {
            ++i;
            uint64_t take = i == weights.size() ? left : std::min<uint64_t>(left, align_up((size_t)(n * w / wsum), 32));
            if (take) plan.emplace_back(pos, take);
            pos += take; left -= take;
        }
    };
    if (nq < 256) { plan.emplace_back(0, nq); return plan; }
    if (nq <= 2048) {
        taper(0, nq, {4, 3, 2, 1});
        return plan;
    }
    for (uint64_t q0 = 0; q0 < nq; q0 += 1024) plan.emplace_back(q0, std::min<uint64_t>(1024, nq - q0));
    return plan;
}

// The per-call decisions of rbq_search_batch on one replica (search_host, api_search.hip), beside the sub-batches above.
// scan_wave = 2 sends batches of at least kScanWaveMinQueries (rbq_search_plan.hpp) to k_scanw; a host call (host buffers; the caller
// waits for the call) only from this many queries per call: every sub-batch of a smaller call takes the short-chain kernel
constexpr uint64_t kHostWaveMinQueries = 4096;
// rbq_search_batch reads page-locked queries in place from this many queries per call (up to 4 queries take the latency-first
// front: a hundred workgroups per query would each read them over PCIe)
constexpr uint64_t kZeroCopyMinQueries = 5;
// ... and up to this many: page-locked queries are read by k_prep where they lie (device-side address of the caller's buffer)
// (measured, GIST-1M shape: 1024 queries per call 297 -> 280 us, 1536: 388 -> 376, 256: 212 -> 198 us; but one query 133 -> 147 us,
// 2048 per call 445 -> 457 and from 4096 the copy engine clearly beats the waves' own PCIe reads: 678 -> 778 us — hence the window)
// (pageable queries, read from the lane's pinned staging buffer: 1024 per call 381 -> 373 us, but 2048 per call 524 -> 591 us:
// there the staged DMA pieces overlap the host copy better than one big copy followed by in-place reads — window <= 1024)
// (round 5: the preparation kernels now request a query's elements eight at a time instead of one per round trip — 15 PCIe round
// trips per query at D = 960 became 2 — and the window opens at 5 queries: 8 per call 149 -> 142 us, 16: 156 -> 149, 24: 161 -> 153)
constexpr uint64_t kZeroCopyMaxPinned = 1536, kZeroCopyMaxPageable = 1024;
// pageable queries, every sub-batch on its own lane (nsub <= nlanes): helper threads stage sub-batches 1.. into their lanes' pinned
// buffers while the calling thread stages and launches sub-batch 0 — at most kMaxHelped sub-batches, calls of at least 512 KB of queries
constexpr uint64_t kMaxHelped = 8;
constexpr uint64_t kHelpersMinBytes = 512u << 10;
struct HostCallOptions {
    uint32_t host_lanes = 0;        // 0 = default (six)
    bool host_zero_copy = true, host_stage_helpers = true;
};
struct HostCallPlan {
    uint32_t nlanes = 0;        // lanes (stream + workspace + pinned staging each) the sub-batches travel through
    bool zero_copy = false;     // the preparation reads the queries from page-locked host memory in place
    bool helpers = false;       // helper threads are wanted for sub-batches 1.. (the caller still has to get them started)
    bool latency_first = false; // every sub-batch takes the short-chain scan kernel
};
inline HostCallPlan host_call_plan(uint64_t nq, bool in_pinned, size_t query_bytes, uint64_t nsub, const HostCallOptions& o) {
    HostCallPlan p;
    p.nlanes = (uint32_t)std::min<uint64_t>(nsub, o.host_lanes ? o.host_lanes : 6u);
    p.zero_copy = o.host_zero_copy && nq >= kZeroCopyMinQueries && nq <= (in_pinned ? kZeroCopyMaxPinned : kZeroCopyMaxPageable);
    p.helpers = !in_pinned && o.host_stage_helpers && nsub >= 2 && nsub <= p.nlanes && nsub <= kMaxHelped && query_bytes >= kHelpersMinBytes;
    p.latency_first = nq < kHostWaveMinQueries;
    return p;
}

// The argument errors of rbq_mstg_search_batch* and rbq_mstg_search_refined_batch* (include/rbq_mstg.h), in their order; no
// device is needed to find any of them.  RBQ_OK with *done set: the call is answered as it stands (nq == 0).
struct MstgSearchArgs {
    bool have_index = false;       // a non-null handle with a replica
    uint64_t n_vectors = 0;
    uint32_t dim = 0, query_dim = 0;
    int rotator = 0;
    uint64_t nq = 0;
    bool queries = false, out_ids = false, out_scores = false, out_counts = false; // which buffers are non-null
    uint32_t top_k = 0;
    bool refined = false;          // rbq_mstg_search_refined_batch*: the pool is max(refine_pool, top_k)
    uint32_t refine_pool = 0;
};
constexpr uint32_t kMstgTopKHardMax = 1u << 20;  // (kTopKHardMax of the device side)
constexpr uint32_t kMstgRefinePoolMax = 4096;    // RBQ_MSTG_REFINE_POOL_MAX
inline int mstg_search_check(const MstgSearchArgs& a, std::string* detail, bool* done, uint32_t* pool) {
    auto fail = [&](int code, const std::string& msg) { if (detail) *detail = msg; return code; };
    if (done) *done = false;
    if (pool) *pool = 0;
    if (!a.have_index) return fail(RBQ_INVALID_CONFIG, "null index");
    if (a.n_vectors == 0) return fail(RBQ_EMPTY_INDEX, "index is empty");
    if (a.query_dim != a.dim) return fail(RBQ_DIMENSION_MISMATCH, "expected " + std::to_string(a.dim) + ", got " + std::to_string(a.query_dim));
    if (a.rotator != RBQ_ROTATOR_NONE) return fail(RBQ_INVALID_CONFIG, "MSTG search needs an index created with rotator NONE");
    if (a.nq == 0) { if (done) *done = true; return RBQ_OK; }
    if (a.nq > 0x7fffffffull) return fail(RBQ_INVALID_CONFIG, "batch too large");
    // (top_k == 0: out_ids and out_scores hold no element, so they have no address to ask for)
    if (!a.queries || !a.out_counts || (a.top_k && (!a.out_ids || !a.out_scores))) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (a.top_k > kMstgTopKHardMax || (uint64_t)std::min<uint64_t>(a.nq, 16384) * ((uint64_t)a.top_k + 1) * 8 > (8ull << 30))
        return fail(RBQ_INVALID_CONFIG, "top_k too large for one call (top_k <= 2^20)");
    if (a.refined) {
        const uint32_t p = std::max(a.refine_pool, a.top_k);
        if (p > kMstgRefinePoolMax)
            return fail(RBQ_INVALID_CONFIG, "refine pool too large: max(refine_pool, top_k) <= " + std::to_string(kMstgRefinePoolMax));
        if (pool) *pool = p;
    }
    return RBQ_OK;
}

// The refined MSTG call with the option mstg_rerank scores its pool exactly against the raw rows attached to
// the replica that serves it: without rows, or with the handle's "rerank" 0, the call is refused — nothing is silently approximated.
// Comes after mstg_search_check's errors and before any kernel launch.  option 0: the call never looks at the rows.
inline int mstg_rerank_check(bool option, bool have_raw, bool rerank_on, std::string* detail) {
    if (!option || (have_raw && rerank_on)) return RBQ_OK;
    if (detail)
        *detail = !have_raw ? "exact MSTG rerank needs raw vectors attached (rbq_index_set_rerank_vectors) or mstg_rerank 0"
                            : "exact MSTG rerank needs the rerank on: set the option rerank 1 or mstg_rerank 0";
    return RBQ_INVALID_CONFIG;
}

} // namespace rbq_host
