// querycheck_main.cpp — stand-alone driver of rbq_host::QueryRows (csrc/host/rbq_host_logic.hpp) for tests/test_query_dtype_host.py
// (compiled there with AddressSanitizer + UBSan).  Input: a text file, one case per line:
//   <dtype> <dim> <nq> <forced sub-batch, 0 = default plan> <replicas>
// Output, one line per case: the row size, then for every replica shard r its first byte and length, then for every sub-batch j of
// the WHOLE call (one replica) its first byte and length — all from QueryRows over shard_range / subbatch_plan, as rbq_search_batch
// computes them — and the answers of aligned() for an even and an odd address:
//   row <bytes> | shards <off>:<len> ... | subs <off>:<len> ... | aligned <0/1> <0/1>
// Every (offset, length) is also walked over a real buffer of nq rows (a byte is read at both ends), so an offset past the buffer
// is a sanitizer report, not only a wrong number.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rbq_host_logic.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: querycheck <cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        int dtype;
        uint32_t dim;
        uint64_t nq, forced, R;
        if (!(s >> dtype >> dim >> nq >> forced >> R) || R == 0) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        const rbq_host::QueryRows qr{dtype, dim};
        std::vector<uint8_t> buf(qr.bytes(nq) + 2, 1); // (+ 2: an odd base for aligned())
        const float* base = (const float*)buf.data();
        unsigned sum = 0;
        auto span = [&](uint64_t q0, uint64_t n) {
            const uint8_t* p = (const uint8_t*)qr.at(base, q0);
            const size_t len = qr.bytes(n);
            if (len) sum += p[0] + p[len - 1];
            std::cout << " " << (size_t)(p - buf.data()) << ":" << len;
        };
        std::cout << "row " << qr.row_bytes() << " | shards";
        for (uint64_t r = 0; r < R; ++r) {
            uint64_t q0, q1;
            rbq_host::shard_range(r, R, nq, &q0, &q1);
            span(q0, q1 - q0);
        }
        std::cout << " | subs";
        for (const auto& sb : rbq_host::subbatch_plan(nq, forced)) span(sb.first, sb.second);
        const bool even = ((uintptr_t)buf.data() & 1u) == 0;
        std::cout << " | aligned " << (int)qr.aligned(buf.data() + (even ? 0 : 1)) << " " << (int)qr.aligned(buf.data() + (even ? 1 : 0));
        std::cout << " | touched " << sum << "\n";
    }
    return 0;
}
