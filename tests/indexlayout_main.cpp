// indexlayout_main.cpp — stand-alone driver of csrc/host/rbq_index_layout.hpp for tests/test_index_layout_host.py (compiled there
// with AddressSanitizer + UBSan).  Input: a text file, one case per line, "<D> <Dc> <ex_bits> | <list sizes>"; a size is a
// number or "<count>*<number>" (that many lists of the size).  Output, one line per case:
//   ok blocks=.. vectors=.. | gb0 .. | block_list .. | block_nv .. | prefix .. | bytes <name>=<value> ..
// (block_list / block_nv: left out above 65536 blocks), or
//   refused <detail>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rbq_index_layout.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: indexlayout <cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        const size_t bar = line.find('|');
        if (bar == std::string::npos) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        uint32_t D = 0, Dc = 0, ex_bits = 0;
        { std::istringstream s(line.substr(0, bar)); if (!(s >> D >> Dc >> ex_bits)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; } }
        std::vector<uint32_t> ln;
        {
            std::istringstream s(line.substr(bar + 1));
            std::string tok;
            while (s >> tok) {
                const size_t star = tok.find('*');
                const uint64_t count = star == std::string::npos ? 1 : std::stoull(tok.substr(0, star));
                const uint64_t v = std::stoull(star == std::string::npos ? tok : tok.substr(star + 1));
                ln.insert(ln.end(), count, (uint32_t)v);
            }
        }
        rbq_host::ListLayout L;
        std::string detail;
        if (!rbq_host::list_layout(ln.data(), ln.size(), &L, &detail)) {
            std::cout << "refused " << detail << "\n";
            continue;
        }
        std::cout << "ok blocks=" << L.blocks << " vectors=" << L.vectors << " | gb0";
        for (uint32_t v : L.gb0) std::cout << " " << v;
        if (L.blocks <= 65536) {
            std::vector<uint32_t> bl, bn;
            rbq_host::block_tables(ln, L.gb0, L.blocks, &bl, &bn);
            std::cout << " | block_list";
            for (uint64_t b = 0; b < L.blocks; ++b) std::cout << " " << bl.at(b);
            std::cout << " | block_nv";
            for (uint64_t b = 0; b < L.blocks; ++b) std::cout << " " << bn.at(b);
        }
        std::cout << " | prefix";
        for (uint64_t v : rbq_host::nblk_desc_prefix(ln)) std::cout << " " << v;
        const rbq_host::IndexBytes B = rbq_host::index_bytes(D, Dc, ex_bits, L.blocks, ln.size());
        const std::pair<const char*, size_t> sizes[] = {
            {"block_stride", B.block_stride}, {"ex_slot", B.ex_slot}, {"slots", B.slots}, {"blocks", B.blocks}, {"ids", B.ids},
            {"ex", B.ex}, {"ex_alloc", B.ex_alloc}, {"fadd_ex", B.fadd_ex}, {"fres_ex", B.fres_ex}, {"bsum", B.bsum}, {"bsumx", B.bsumx},
            {"lsum", B.lsum}, {"delta", B.delta}, {"vl", B.vl}, {"rnorm", B.rnorm}, {"centroids", B.centroids}, {"cent_hl", B.cent_hl},
            {"cent_f16", B.cent_f16}, {"cent_f16_resid", B.cent_f16_resid}, {"cnorm2", B.cnorm2}, {"list_gb0", B.list_gb0},
            {"list_n", B.list_n}};
        std::cout << " | bytes";
        for (const auto& kv : sizes) std::cout << " " << kv.first << "=" << kv.second;
        std::cout << "\n";
    }
    return 0;
}
