// removecheck_main.cpp — stand-alone driver of csrc/host/rbq_remove_plan.hpp for tests/test_remove_plan_host.py (compiled there
// with AddressSanitizer + UBSan).  Input: a text file, one case per line, in one of two forms:
//   P <old sizes> | <removed positions>   positions count the vectors of all lists in (list, in-list position) order; the program
//                                         builds the keep mask of every old block, scans the kept counts, plans, and maps every
//                                         kept slot with remove_rank / remove_dst_slot, as the kernels do
//   K <old sizes> | <kept counts>         the plan alone (the 32-bit limits, where masks would not fit in memory)
// Output, one line per case:
//   ok old_blocks=.. new_blocks=.. old_vectors=.. new_vectors=.. | new_n .. | new_gb0 .. | old_gb0 .. [| map ..]
// (map: the old slot moved into every slot of the shrunk index, -1 for a pad), or
//   refused <detail>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rbq_remove_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: removecheck <cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        const size_t bar = line.find('|');
        if (bar == std::string::npos || line.size() < 2 || (line[0] != 'P' && line[0] != 'K')) {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        const bool positions = line[0] == 'P';
        std::vector<uint32_t> old_n, kept;
        std::vector<uint64_t> second;
        { std::istringstream s(line.substr(1, bar - 1)); uint64_t v; while (s >> v) old_n.push_back((uint32_t)v); }
        { std::istringstream s(line.substr(bar + 1)); uint64_t v; while (s >> v) second.push_back(v); }
        const size_t nl = old_n.size();
        std::vector<uint32_t> mask, scan, block_list, gb0;
        if (positions) {
            // the keep mask of every old block (real slots minus the removed positions) and the exclusive scan of the kept counts
            uint64_t nb = 0, nv = 0;
            for (size_t c = 0; c < nl; ++c) {
                gb0.push_back((uint32_t)nb);
                for (uint32_t j = 0; j < (old_n[c] + 31u) / 32u; ++j) {
                    const uint32_t real = old_n[c] - j * 32u < 32u ? old_n[c] - j * 32u : 32u;
                    mask.push_back(real == 32u ? 0xffffffffu : (1u << real) - 1u);
                    block_list.push_back((uint32_t)c);
                }
                nb += (old_n[c] + 31u) / 32u; nv += old_n[c];
            }
            for (uint64_t p : second) {
                if (p >= nv) { std::fprintf(stderr, "bad position: %s\n", line.c_str()); return 2; }
                size_t c = 0;
                uint64_t base = 0;
                while (p - base >= old_n[c]) { base += old_n[c]; ++c; }
                const uint64_t q = p - base;
                mask.at(gb0[c] + q / 32u) &= ~(1u << (q % 32u));
            }
            scan.assign(nb + 1, 0);
            for (uint64_t b = 0; b < nb; ++b) scan[b + 1] = scan[b] + (uint32_t)__builtin_popcount(mask[b]);
            for (size_t c = 0; c < nl; ++c) kept.push_back(scan.at(gb0[c] + (old_n[c] + 31u) / 32u) - scan.at(gb0[c]));
        } else {
            if (second.size() != nl) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
            for (uint64_t v : second) kept.push_back((uint32_t)v);
        }
        rbq_host::RemovePlan p;
        std::string detail;
        if (!rbq_host::remove_plan(old_n.data(), kept.data(), nl, &p, &detail)) {
            std::cout << "refused " << detail << "\n";
            continue;
        }
        std::cout << "ok old_blocks=" << p.old_blocks << " new_blocks=" << p.new_blocks << " old_vectors=" << p.old_vectors
                  << " new_vectors=" << p.new_vectors;
        const std::vector<uint32_t>* arrs[3] = {&p.new_n, &p.new_gb0, &p.old_gb0};
        const char* names[3] = {"new_n", "new_gb0", "old_gb0"};
        for (int a = 0; a < 3; ++a) {
            std::cout << " | " << names[a];
            for (uint32_t v : *arrs[a]) std::cout << " " << v;
        }
        if (positions) {
            // the slot map exactly as k_remove_slot_map scatters it: pads keep the fill
            std::vector<uint32_t> map(p.new_blocks * 32u, rbq_host::kRemoveNoSlot);
            for (uint64_t i = 0; i < p.old_blocks * 32u; ++i) {
                const uint32_t b = (uint32_t)(i / 32u), lane = (uint32_t)(i % 32u), m = mask.at(b);
                if (!((m >> lane) & 1u)) continue;
                const uint32_t c = block_list.at(b);
                const uint32_t dst = rbq_host::remove_dst_slot(p.new_gb0.at(c), rbq_host::remove_rank(scan.at(b), scan.at(p.old_gb0.at(c)), m, lane));
                if (map.at(dst) != rbq_host::kRemoveNoSlot) { std::fprintf(stderr, "slot %u written twice\n", dst); return 3; }
                map.at(dst) = (uint32_t)i;
            }
            std::cout << " | map";
            for (uint32_t v : map) std::cout << " " << (v == rbq_host::kRemoveNoSlot ? -1ll : (long long)v);
        }
        std::cout << "\n";
    }
    return 0;
}
