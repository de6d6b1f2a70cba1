// bfplancheck_main.cpp — stand-alone driver of rbq_host::plan_bf_call (csrc/host/rbq_bf_plan.hpp) for tests/test_bf_plan_host.py
// (compiled there with AddressSanitizer + UBSan).
// Input: a text file, one case per line:   <n> <nq> <range 0|1> <top_k or capacity> <chunk_vectors>
// Output, one line per case:               nv_chunk= n_chunks= sub= lds_heap= heap_ws= cap= spans=
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "rbq_bf_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: bfplancheck <cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        rbq_host::BfCallShape sh;
        int range;
        if (!(s >> sh.n >> sh.nq >> range >> sh.top_k >> sh.chunk_vectors)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        sh.range = range != 0;
        const rbq_host::BfCallPlan p = rbq_host::plan_bf_call(sh);
        std::cout << "nv_chunk=" << p.nv_chunk << " n_chunks=" << p.n_chunks << " sub=" << p.sub << " lds_heap=" << p.lds_heap
                  << " heap_ws=" << p.heap_ws << " cap=" << p.cap << " spans=" << p.spans << "\n";
    }
    return 0;
}
