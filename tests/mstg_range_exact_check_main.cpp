// The verdict of rbq_host::mstg_range_exact_check (rbq_host_logic.hpp) for all sixteen combinations, one line
// each: option distinct have_raw rerank_on rc detail.  Built with ASan + UBSan and run by tests/test_mstg_range_exact_host.py.
#include <cstdio>
#include <string>

#include "rbq.h"
#include "rbq_host_logic.hpp"

int main() {
    for (int m = 0; m < 16; ++m) {
        const bool option = (m & 8) != 0, distinct = (m & 4) != 0, have_raw = (m & 2) != 0, rerank_on = (m & 1) != 0;
        std::string detail;
        const int rc = rbq_host::mstg_range_exact_check(option, distinct, have_raw, rerank_on, &detail);
        if (rc != rbq_host::mstg_range_exact_check(option, distinct, have_raw, rerank_on, nullptr)) return 2; // (the detail is optional)
        std::printf("%d %d %d %d %d %s\n", (int)option, (int)distinct, (int)have_raw, (int)rerank_on, rc, detail.c_str());
    }
    return 0;
}
