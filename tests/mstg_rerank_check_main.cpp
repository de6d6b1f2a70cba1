// mstg_rerank_check_main.cpp — prints the verdict of rbq_host::mstg_rerank_check (csrc/host/rbq_host_logic.hpp)
// for all eight combinations of (option, raw vectors attached, rerank on), one line each:
//   option have_raw rerank_on rc detail
// Built with AddressSanitizer + UBSan and run as a child process by tests/test_mstg_rerank_host.py.
#include <cstdio>
#include <string>

#include "rbq.h"
#include "rbq_host_logic.hpp"

int main() {
    for (int m = 0; m < 8; ++m) {
        const bool option = (m & 4) != 0, have_raw = (m & 2) != 0, rerank_on = (m & 1) != 0;
        std::string detail;
        const int rc = rbq_host::mstg_rerank_check(option, have_raw, rerank_on, &detail);
        const int rc_null = rbq_host::mstg_rerank_check(option, have_raw, rerank_on, nullptr); // (the detail is optional)
        if (rc != rc_null) return 2;
        std::printf("%d %d %d %d %s\n", (int)option, (int)have_raw, (int)rerank_on, rc, detail.c_str());
    }
    return 0;
}
