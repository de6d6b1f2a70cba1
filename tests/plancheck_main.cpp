// plancheck_main.cpp — stand-alone driver of rbq_host::plan_search (csrc/host/rbq_search_plan.hpp) and rbq_host::host_call_plan
// (csrc/host/rbq_host_logic.hpp) for tests/test_search_plan_host.py (compiled there with AddressSanitizer + UBSan).
// Input: a text file, one case per line.
//   plan <key>=<value> ...     a device search call; keys: the fields of SearchShape and RouteOptions by name (missing: the default),
//                              and bpl = blocks per list of the prefix-sum table the plan clamps nprobe against (a real array of
//                              n_lists + 1 entries: an index past it is a sanitizer report)
//   host <nq> <in_pinned> <query_bytes> <nsub> <host_lanes> <host_zero_copy> <host_stage_helpers>
// Output, one line per case:
//   nprobe= big_nprobe= wl_stride= prep= rank= tile= ksplit= planar= select= lazy= heap_global= wave= tie= tie_cap= rot_hl= rot_f16=
//   resid= planes= keywin= ok=        (ok: plan_search_ok)
//   lanes= zero_copy= helpers= latency_first=
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "rbq_host_logic.hpp"
#include "rbq_search_plan.hpp"

using namespace rbq_host;

static const char* prep_name(PrepForm f) {
    switch (f) {
        case PrepForm::none: return "none";
        case PrepForm::prep: return "prep";
        case PrepForm::prep_wave: return "prep_wave";
        case PrepForm::wg: return "wg";
        case PrepForm::wg_zero: return "wg_zero";
        case PrepForm::lat_scorers: return "lat_scorers";
    }
    return "?";
}
static const char* rank_name(RankRoute r) {
    switch (r) {
        case RankRoute::none: return "none";
        case RankRoute::exact: return "exact";
        case RankRoute::f32: return "f32";
        case RankRoute::bf16x3: return "bf16x3";
        case RankRoute::f16: return "f16";
    }
    return "?";
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: plancheck <cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    std::vector<uint64_t> prefix;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        if (kind == "host") {
            uint64_t nq, query_bytes, nsub;
            int pinned, lanes, zc, helpers;
            if (!(s >> nq >> pinned >> query_bytes >> nsub >> lanes >> zc >> helpers)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
            HostCallOptions o;
            o.host_lanes = (uint32_t)lanes; o.host_zero_copy = zc != 0; o.host_stage_helpers = helpers != 0;
            const HostCallPlan p = host_call_plan(nq, pinned != 0, (size_t)query_bytes, nsub, o);
            std::cout << "lanes=" << p.nlanes << " zero_copy=" << p.zero_copy << " helpers=" << p.helpers << " latency_first=" << p.latency_first << "\n";
            continue;
        }
        if (kind != "plan") { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        std::map<std::string, long long> kv;
        std::string tok;
        while (s >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { std::fprintf(stderr, "bad token: %s\n", tok.c_str()); return 2; }
            kv[tok.substr(0, eq)] = std::stoll(tok.substr(eq + 1), nullptr, 0);
        }
        auto take = [&](const char* k, long long dflt) {
            auto it = kv.find(k);
            if (it == kv.end()) return dflt;
            const long long v = it->second;
            kv.erase(it);
            return v;
        };
        SearchShape sh;
        RouteOptions o;
        sh.nq = (uint64_t)take("nq", 1); sh.call_nq = (uint64_t)take("call_nq", 0); sh.top_k = (uint32_t)take("top_k", 10);
        sh.nprobe = (uint32_t)take("nprobe", 16); sh.n_lists = (uint64_t)take("n_lists", 64); sh.D = (uint32_t)take("D", 64);
        sh.Dc = (sh.D + 63u) / 64u * 64u;
        sh.rotator = (int)take("rotator", 1); sh.ex_bits = (uint32_t)take("ex_bits", 0); sh.rank_f16_ok = take("rank_f16_ok", 1) != 0;
        sh.has_filter = take("has_filter", 0) != 0; sh.has_diag = take("has_diag", 0) != 0; sh.range = take("range", 0) != 0;
        sh.latency_first = take("latency_first", 0) != 0; sh.mstg = take("mstg", 0) != 0; sh.probe_installed = take("probe_installed", 0) != 0;
        const uint64_t bpl = (uint64_t)take("bpl", 3);
        o.exact_rank = take("exact_rank", 0) != 0; o.f32_rank = take("f32_rank", 0) != 0; o.wg_prep = take("wg_prep", 0) != 0;
        o.latency_path = (int)take("latency_path", 1); o.rank_ksplit = (int)take("rank_ksplit", 1); o.rank_tile = (int)take("rank_tile", 0);
        o.rank_f16 = (int)take("rank_f16", -1); o.rank_planar = take("rank_planar", 0) != 0; o.stage_mask = (uint32_t)take("stage_mask", 0xf);
        o.lazy_select = take("lazy_select", 1) != 0; o.lazy_filter = take("lazy_filter", 1) != 0; o.head_exact = take("head_exact", 1) != 0;
        o.no_block_bound = take("no_block_bound", 0) != 0; o.scan_wave = (int)take("scan_wave", 2); o.tie_log = take("tie_log", 1) != 0;
        o.tie_log_cap = (uint32_t)take("tie_log_cap", 0); o.exact_heap = take("exact_heap", 0) != 0;
        if (!kv.empty()) { std::fprintf(stderr, "unknown key %s in: %s\n", kv.begin()->first.c_str(), line.c_str()); return 2; }
        if (!sh.mstg) {
            prefix.resize(sh.n_lists + 1); // exactly what an index holds
            for (uint64_t i = 0; i <= sh.n_lists; ++i) prefix[i] = i * bpl;
            sh.nblk_desc_prefix = prefix.data(); sh.nblk_desc_prefix_len = prefix.size();
        }
        const SearchPlan p = plan_search(sh, o);
        std::cout << "nprobe=" << p.nprobe << " big_nprobe=" << p.big_nprobe << " wl_stride=" << p.wl_stride << " prep=" << prep_name(p.prep)
                  << " rank=" << rank_name(p.rank) << " tile=" << p.tile << " ksplit=" << p.ksplit << " planar=" << p.planar
                  << " select=" << (p.exact_select ? "exact" : "mfma") << " lazy=" << p.lazy << " heap_global=" << p.heap_in_global
                  << " wave=" << p.wave_kernel << " tie=" << p.tie_log << " tie_cap=" << p.tie_log_cap << " rot_hl=" << p.need_rot_hl
                  << " rot_f16=" << p.need_rot_f16 << " resid=" << p.need_rank_resid << " planes=" << p.need_rank_planes
                  << " keywin=" << p.need_key_window << " ok=" << plan_search_ok(p, sh, o) << "\n";
    }
    return 0;
}
