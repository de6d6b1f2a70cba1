// loadcheck_main.cpp — the GPU-free half of rbq_index_load_rbq1_stream (csrc/host/rbq_load_stream.hpp) against rbq1_parse, as a
// stand-alone program: tests/test_load_stream_host.py compiles it with -fsanitize=address,undefined and runs it as a child
// process.  TEST INFRASTRUCTURE: host code only, not linked into the product.
//
//   loadcheck <list file> <span bytes>...
// The list file names one stream file per line.  For every stream and span size the program runs the framing pass over a
// reader of the file, cuts the spans, checks the ex-code prefixes with the plain loop that stands in for the GPU, checksums
// the spans on the host, joins the CRCs with crc32_combine and asks for the verdict; then it parses the same bytes with
// rbq1_parse.  Every span is read into a heap block of exactly its size, so a piece that leaves its span is an ASan report.
// Output, one line per (stream, span):
//   <file> span=<n> stream rc=<rc> detail=<detail> | parse rc=<rc> detail=<detail> | lists=<k> <off>:<n> ... | <AGREE or DIFFER>
// Exit status: 0 when every line agrees and the pieces of every complete stream tile the cluster region exactly once.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>

#include "rbq_load_stream.hpp"

using namespace rbq_host;

static bool slurp(const std::string& path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct Answer { int rc = 0; std::string detail; };

// returns false when an internal check failed (message on stderr)
static bool run_stream(const std::vector<uint8_t>& file, uint64_t span_req, Answer& ans, LoadFraming& F) {
    const uint64_t total = file.size();
    bool ok = true;
    auto rd = [&](uint64_t off, void* dst, uint64_t n) {
        if (!load_fits(off, n, total)) { std::fprintf(stderr, "read outside the stream: %llu + %llu\n", (unsigned long long)off, (unsigned long long)n); ok = false; return false; }
        std::memcpy(dst, file.data() + off, n);
        return true;
    };
    if (!load_frame(rd, total, F)) { ans.rc = RBQ_IO; ans.detail = "read callback failed"; return false; }
    bool want_stored = false;
    if (!F.header_ok) {
        ans.rc = load_verdict_framing(F, kLoadNoBadPrefix, total, &ans.detail, &want_stored);
        return ok;
    }
    const uint64_t budget = load_span_budget(span_req, F.g);
    uint32_t crc = 0;
    if (F.complete()) crc = crc32_update(0, file.data() + 8, F.cluster_begin - 8);
    LoadCutter cut(F, budget);
    std::vector<LoadPiece> pieces;
    uint64_t s_off = 0, s_len = 0, bad = kLoadNoBadPrefix, covered = F.cluster_begin;
    while (cut.next(pieces, &s_off, &s_len)) {
        if (s_off != covered) { std::fprintf(stderr, "span at %llu, expected %llu\n", (unsigned long long)s_off, (unsigned long long)covered); ok = false; }
        if (s_len > budget || pieces.size() > kLoadMaxPieces) { std::fprintf(stderr, "span of %llu bytes over budget\n", (unsigned long long)s_len); ok = false; }
        if (s_off % 4 != 0 && F.g.D % 16 == 0) { std::fprintf(stderr, "span not at a multiple of 4\n"); ok = false; }
        std::unique_ptr<uint8_t[]> span(new uint8_t[s_len]); // exact size: ASan guards both ends
        if (!rd(s_off, span.get(), s_len)) return false;
        // the pieces tile the span: each starts where the one before ended, the last ends with the span
        uint64_t at = 0;
        for (const LoadPiece& p : pieces) {
            if (p.off != at) { std::fprintf(stderr, "piece at %llu, expected %llu\n", (unsigned long long)p.off, (unsigned long long)at); ok = false; }
            at = p.off + (uint64_t)p.count * F.g.unit(p.kind);
            if (at > s_len) { std::fprintf(stderr, "piece crosses its span\n"); ok = false; }
            if (!p.count) { std::fprintf(stderr, "empty piece\n"); ok = false; }
        }
        if (at != s_len) { std::fprintf(stderr, "pieces end at %llu of %llu\n", (unsigned long long)at, (unsigned long long)s_len); ok = false; }
        const uint64_t nwg = load_assign_workgroups(pieces, F.h.ex_bits, F.complete());
        if (!pieces.empty() && pieces.back().wg0 > nwg) ok = false;
        const uint64_t b = load_check_prefixes(span.get(), s_off, pieces, F.g);
        bad = std::min(bad, b);
        if (F.complete()) crc = crc32_combine(crc, crc32_ieee(span.get(), s_len), s_len);
        covered = s_off + s_len;
    }
    if (F.complete() && covered != F.body_end) { std::fprintf(stderr, "spans end at %llu, body at %llu\n", (unsigned long long)covered, (unsigned long long)F.body_end); ok = false; }
    if (covered > F.region_end) { std::fprintf(stderr, "spans leave the region\n"); ok = false; }
    ans.rc = load_verdict_framing(F, bad, total, &ans.detail, &want_stored);
    if (ans.rc == RBQ_OK) {
        uint32_t stored = 0;
        if (!rd(F.body_end, &stored, 4)) return false;
        ans.rc = load_verdict_crc(crc, stored, &ans.detail);
    }
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: loadcheck <list file> <span bytes>...\n"); return 2; }
    std::ifstream lf(argv[1]);
    std::string path;
    int status = 0;
    while (std::getline(lf, path)) {
        if (path.empty()) continue;
        std::vector<uint8_t> heap;
        if (!slurp(path, heap)) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        // an exact-size copy for rbq1_parse (a vector's capacity may hide an overrun)
        std::unique_ptr<uint8_t[]> exact(new uint8_t[heap.size() ? heap.size() : 1]);
        if (!heap.empty()) std::memcpy(exact.get(), heap.data(), heap.size());
        Answer want;
        rbq_header h;
        std::vector<ListSrc> lists;
        want.rc = rbq1_parse(exact.get(), heap.size(), &h, &lists, &want.detail);
        for (int a = 2; a < argc; ++a) {
            const uint64_t span = std::strtoull(argv[a], nullptr, 10);
            Answer got;
            LoadFraming F;
            const bool ok = run_stream(heap, span, got, F);
            bool agree = ok && got.rc == want.rc && got.detail == want.detail;
            if (agree && want.rc == RBQ_OK) { // the per-list table against the parser's views
                agree = F.list_n.size() == lists.size();
                for (size_t c = 0; agree && c < lists.size(); ++c)
                    agree = F.list_n[c] == lists[c].n && F.list_off[c] == (uint64_t)(lists[c].centroid - exact.get());
            }
            std::cout << path << " span=" << span << " stream rc=" << got.rc << " detail=" << got.detail << " | parse rc=" << want.rc
                      << " detail=" << want.detail << " | lists=" << F.list_n.size();
            for (size_t c = 0; c < F.list_n.size(); ++c) std::cout << ' ' << F.list_off[c] << ':' << F.list_n[c];
            std::cout << " | " << (agree ? "AGREE" : "DIFFER") << '\n';
            if (!agree) status = 1;
        }
    }
    return status;
}
