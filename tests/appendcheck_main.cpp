// appendcheck_main.cpp — stand-alone driver of csrc/host/rbq_append_plan.hpp for tests/test_append_plan_host.py (compiled there
// with AddressSanitizer + UBSan).  Input: a text file, one case per line, "<old sizes> | <added counts>" (two lists of the same
// length, space separated).  Output, one line per case:
//   ok old_blocks=.. new_blocks=.. new_vectors=.. | new_n .. | new_gb0 .. | old_gb0 .. | cursor .. | src ..
// (src: the old block carried into every block of the grown index, -1 for none; left out above 65536 blocks), or
//   refused <detail>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rbq_append_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: appendcheck <cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        const size_t bar = line.find('|');
        if (bar == std::string::npos) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        std::vector<uint32_t> old_n;
        std::vector<uint64_t> added;
        { std::istringstream s(line.substr(0, bar)); uint64_t v; while (s >> v) old_n.push_back((uint32_t)v); }
        { std::istringstream s(line.substr(bar + 1)); uint64_t v; while (s >> v) added.push_back(v); }
        if (old_n.size() != added.size()) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        rbq_host::AppendPlan p;
        std::string detail;
        if (!rbq_host::append_plan(old_n.data(), added.data(), old_n.size(), &p, &detail)) {
            std::cout << "refused " << detail << "\n";
            continue;
        }
        std::cout << "ok old_blocks=" << p.old_blocks << " new_blocks=" << p.new_blocks << " new_vectors=" << p.new_vectors;
        const std::vector<uint32_t>* arrs[4] = {&p.new_n, &p.new_gb0, &p.old_gb0, &p.cursor};
        const char* names[4] = {"new_n", "new_gb0", "old_gb0", "cursor"};
        for (int a = 0; a < 4; ++a) {
            std::cout << " | " << names[a];
            for (uint32_t v : *arrs[a]) std::cout << " " << v;
        }
        if (p.new_blocks <= 65536) {
            // block -> list exactly as upload_block_tables lays it out, then the kernel's rule per block
            std::vector<long long> src(p.new_blocks, -2);
            for (size_t c = 0; c < old_n.size(); ++c) {
                const uint32_t nb = p.new_n[c] / 32u + (p.new_n[c] % 32u ? 1u : 0u);
                for (uint32_t j = 0; j < nb; ++j) {
                    const uint32_t b = p.new_gb0[c] + j, s = rbq_host::append_src_block(b, p.new_gb0[c], p.old_gb0[c], old_n[c]);
                    src.at(b) = s == rbq_host::kAppendNoBlock ? -1 : (long long)s;
                }
            }
            std::cout << " | src";
            for (long long v : src) std::cout << " " << v;
        }
        std::cout << "\n";
    }
    return 0;
}
