"""The routing plan of a device search call (rbq_host::plan_search, csrc/host/rbq_search_plan.hpp) and the
per-call decisions of rbq_search_batch (rbq_host::host_call_plan), checked without a GPU: a stand-alone program under
AddressSanitizer + UBSan (tests/plancheck_main.cpp) prints the plan of every case — nothing sanitized is loaded into this process.

Expected values come from two sources that do not read the new function: a table spelt out by hand, and `parent_route`, the
routing conditions as the three host functions wrote them out before the plan existed (duplicated conditions and all)."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

K_NPROBE_MAX, K_TOPK_MAX, K_TOPK_REG_MAX, K_LDS_MAX = 8192, 16384, 256, 160 * 1024
LAT_MAX_BYTES = 96 << 20

SHAPE_DEFAULTS = dict(nq=1, call_nq=0, top_k=10, nprobe=16, n_lists=64, D=64, rotator=1, ex_bits=0, rank_f16_ok=1, has_filter=0,
                      has_diag=0, range=0, latency_first=0, mstg=0, probe_installed=0, bpl=3)
OPT_DEFAULTS = dict(exact_rank=0, f32_rank=0, wg_prep=0, latency_path=1, rank_ksplit=1, rank_tile=0, rank_f16=-1, rank_planar=0,
                    stage_mask=0xf, lazy_select=1, lazy_filter=1, head_exact=1, no_block_bound=0, scan_wave=2, tie_log=1, tie_log_cap=0,
                    exact_heap=0)


@pytest.fixture(scope="module")
def plancheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plancheck") / "plancheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "plancheck_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run_lines(exe, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_text("".join(l + "\n" for l in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(lines)
    return [dict(tok.split("=") for tok in r.split()) for r in rows]


def plan_line(case):
    return "plan " + " ".join("%s=%d" % kv for kv in case.items())


# ---- the parent's routing, restated from search_front / search_core / scan_stage as they stood ------------------------------------
def scan_lds_bytes(Dc, D, ex_bits, top_k):
    """scan_lds_bytes at kNScan 3, kFillK 2: 192 candidates per tile, a queue of 512, 256 threads"""
    if ex_bits:
        cpu = 128 // ex_bits
        qlen = max((D // 16 + cpu - 1) // cpu * cpu * 16, D)
    else:
        qlen = D
    return Dc * 4 + qlen * 4 + (top_k + 1) * 8 + 192 * 2 * 20 + 192 * 4 + 2 * 6 * 4 + 512 * 8 + 3 * 2 * 8 + 32 + 16 * 8


def parent_route(c):
    c = {**SHAPE_DEFAULTS, **OPT_DEFAULTS, **c}
    nq, nlist, D = c["nq"], c["n_lists"], c["D"]
    Dc = (D + 63) // 64 * 64
    r = {}
    # scan_stage (range_stage: no wave kernel, no tie log, no heap workspace)
    wave = c["scan_wave"] == 1 or (c["scan_wave"] == 2 and nq >= 128 and not c["no_block_bound"] and not c["latency_first"])
    tie, cap = False, 0
    if (c["tie_log"] and not wave and not c["has_diag"] and not c["mstg"] and 1 <= c["top_k"] <= K_TOPK_REG_MAX and not c["exact_heap"]
            and not c["probe_installed"]):
        cap_ = c["tie_log_cap"] or (2048 if c["top_k"] < 64 else 8192)
        if nq * cap_ * 12 <= 1 << 30:
            tie, cap = True, cap_
    heap = c["top_k"] > K_TOPK_MAX or scan_lds_bytes(Dc, D, 0 if c["mstg"] else c["ex_bits"], c["top_k"]) > K_LDS_MAX
    if c["range"]:
        wave, tie, cap, heap = False, False, 0, False
    r.update(wave=wave, tie=tie, tie_cap=cap, heap_global=heap)
    if c["mstg"]:
        return r
    # search_front
    nprobe = min(max(c["nprobe"], 1), nlist)
    big_nprobe = nprobe > K_NPROBE_MAX
    split_rank = not c["exact_rank"] and not c["f32_rank"] and D % 64 == 0
    smask = c["stage_mask"]
    call = c["call_nq"] or nq
    ksplit = 1
    if (c["rank_ksplit"] and c["latency_path"] and nq <= 512 and call <= 256 and c["rotator"] != 0 and not c["wg_prep"] and D % 16 == 0
            and split_rank and not c["exact_rank"] and not big_nprobe and smask == 0xf):
        T = 128 if ((((nlist + 127) // 128) * ((nq + 127) // 128) >= 192 and c["rank_tile"] != 64) or c["rank_tile"] == 128) else 64
        tiles = ((nlist + T - 1) // T) * ((nq + T - 1) // T)
        ksplit = 1 if tiles >= 512 else 2 if tiles >= 256 else 4
        while ksplit > 1 and (D // 32) // ksplit < 6:
            ksplit >>= 1
        if c["rank_ksplit"] > 1:
            ksplit = min(c["rank_ksplit"], 4)
    lat_front = bool(c["latency_path"] and nq <= 4 and c["rotator"] != 0 and not c["wg_prep"] and not c["exact_rank"] and not big_nprobe
                     and not c["f32_rank"] and nlist * D * 4 * nq <= LAT_MAX_BYTES and D % 16 == 0 and smask == 0xf)
    tiles128 = ((nlist + 127) // 128) * ((nq + 127) // 128)
    tiles256 = ((nlist + 255) // 256) * ((nq + 127) // 128)
    f16_possible = c["rank_f16_ok"] and split_rank and ksplit == 1 and not c["rank_planar"] and not big_nprobe and not lat_front
    rank_f16 = bool(c["rank_f16"] != 0 and f16_possible
                    and (c["rank_f16"] > 0 or (c["rank_tile"] == 0 and (tiles128 >= 192 or tiles256 >= 2048) and D >= 256)))
    if lat_front:
        prep = "lat_scorers"
    elif c["latency_path"] and nq <= 512 and c["rotator"] != 0 and not c["wg_prep"] and D % 16 == 0:
        prep = "wg_zero" if ksplit > 1 else "wg"
    else:
        prep = "prep" if (c["rotator"] == 0 or c["wg_prep"]) else "prep_wave"  # launch_prep
    big = tiles128 >= 192
    wide = c["rank_tile"] == 256 or (c["rank_tile"] == 0 and tiles256 >= 2048)
    if c["rank_tile"] == 64:
        big = False
    if c["rank_tile"] == 128:
        big = True
    exact = bool(c["exact_rank"] or big_nprobe)
    rank = "exact" if exact else "none" if lat_front else "f32" if not split_rank else "f16" if rank_f16 else "bf16x3"
    gemm_wide = split_rank and wide  # launch_rank_gemm: the 256 grid, which has no z
    lazy_with_filter = c["lazy_filter"] and c["head_exact"] and not c["has_diag"]
    lazy = bool(c["lazy_select"] and (not c["has_filter"] or lazy_with_filter) and not c["no_block_bound"] and not c["range"])
    planar = bool(not exact and not lat_front and split_rank and c["rank_planar"] and not c["probe_installed"])
    if rank not in ("none", "exact"):  # (else no GEMM runs: the tile is nobody's)
        r.update(tile=256 if gemm_wide else 128 if big else 64)
    r.update(nprobe=nprobe, big_nprobe=big_nprobe, wl_stride=max(c["bpl"] * nprobe, 1), prep=prep, rank=rank,
             ksplit=1 if (gemm_wide or lat_front) else ksplit, planar=planar,
             select="exact" if exact else "mfma", lazy=lazy and not exact,  # (k_select never read the flag)
             rot_hl=split_rank, rot_f16=rank_f16, resid=rank_f16, planes=planar, keywin=big_nprobe)
    return r


def same(got, want):
    for k, v in want.items():
        g = got[k]
        if isinstance(v, bool):
            v = int(v)
        if str(v) != g:
            return "%s: plan says %s, expected %s" % (k, g, v)
    return None


# ---- 1. the table spelt out by hand -------------------------------------------------------------------------------------------------
GIST = dict(n_lists=4096, D=960, ex_bits=6)  # FHT-Kac
BIGCALL = dict(n_lists=24576, D=960, ex_bits=6, nq=128, call_nq=1024)  # 192 x 1 tiles of 128, a sub-batch of a large host call

TABLE = [
    # the issue's two examples: 64 x 2 = 128 tiles of 64 -> 4 parts of 30 / 4 = 7 slabs; at D 128 a part would have 1 slab
    (dict(GIST, nq=65), dict(prep="wg_zero", rank="bf16x3", tile=64, ksplit=4, select="mfma", lazy=1, wave=0, tie=1, tie_cap=2048, rot_hl=1)),
    (dict(GIST, nq=65, D=128), dict(prep="wg", rank="bf16x3", tile=64, ksplit=1)),
    # latency front: 4 / 5 queries
    (dict(GIST, nq=4), dict(prep="lat_scorers", rank="none", ksplit=1, select="mfma")),
    (dict(GIST, nq=5), dict(prep="wg_zero", rank="bf16x3", ksplit=4)),
    # ... and n_lists x D x 4 x nq at kLatMaxBytes: 6144 x 1024 x 4 x 4 = 96 MiB exactly, one list more is beyond
    (dict(n_lists=6144, D=1024, nq=4), dict(prep="lat_scorers", rank="none")),
    (dict(n_lists=6145, D=1024, nq=4), dict(prep="wg_zero", rank="bf16x3", ksplit=4)),
    # scan wave: 127 / 128 queries (k_scanw logs no ties); a host call that waits keeps k_scan
    (dict(GIST, nq=127), dict(wave=0, tie=1)),
    (dict(GIST, nq=128), dict(wave=1, tie=0)),
    (dict(GIST, nq=128, latency_first=1), dict(wave=0, tie=1)),
    # workgroup preparation: 512 / 513 queries (a 512-query call is above the split-K bound)
    (dict(GIST, nq=512), dict(prep="wg", ksplit=1, rank="bf16x3", tile=64)),
    (dict(GIST, nq=513), dict(prep="prep_wave", ksplit=1)),
    # split-K: the CALL at 256 / 257 queries
    (dict(GIST, nq=64, call_nq=256), dict(prep="wg_zero", ksplit=4)),
    (dict(GIST, nq=64, call_nq=257), dict(prep="wg", ksplit=1)),
    # split-K parts: 254 / 256 / 510 / 512 tiles of 64 (65 queries: 2 rows)
    (dict(GIST, nq=65, n_lists=8128), dict(ksplit=4)),
    (dict(GIST, nq=65, n_lists=8192), dict(ksplit=2, prep="wg_zero")),
    (dict(GIST, nq=65, n_lists=16320), dict(ksplit=2)),
    (dict(GIST, nq=65, n_lists=16384), dict(ksplit=1, prep="wg")),
    # ... at least six slabs per part: D / 32 / 4 = 6 at D 768, 5 at D 704 (-> 2 parts of 11)
    (dict(GIST, nq=65, D=768), dict(ksplit=4)),
    (dict(GIST, nq=65, D=704), dict(ksplit=2)),
    # big: 191 / 192 tiles of 128; from 192 the f16 product by rule (D >= 256)
    (dict(BIGCALL, n_lists=24448), dict(tile=64, rank="bf16x3", rot_f16=0)),
    (dict(BIGCALL), dict(tile=128, rank="f16", rot_f16=1, resid=1, ksplit=1, prep="wg")),
    # ... the same big call as a device call of 128 queries is split in 4 (192 tiles of 128), which rules the f16 product out
    (dict(BIGCALL, call_nq=0), dict(tile=128, rank="bf16x3", ksplit=4, prep="wg_zero")),
    # the f16 rule: D 192 / 256
    (dict(BIGCALL, D=192), dict(tile=128, rank="bf16x3")),
    (dict(BIGCALL, D=256), dict(tile=128, rank="f16")),
    (dict(BIGCALL, rank_f16_ok=0), dict(tile=128, rank="bf16x3")),
    # wide: 2047 (23 x 89) / 2048 (16 x 128) tiles of 256 x 128, and cfg5
    (dict(n_lists=89 * 256, D=960, nq=23 * 128), dict(tile=128, rank="f16", prep="prep_wave", wave=1)),
    (dict(n_lists=32768, D=960, nq=2048), dict(tile=256, rank="f16")),
    (dict(n_lists=65536, D=960, nq=16384), dict(tile=256, rank="f16", ksplit=1, prep="prep_wave")),
    # nprobe: clamped to [1, n_lists]; at kNprobeMax and beyond
    (dict(GIST, nprobe=0), dict(nprobe=1, wl_stride=3)),
    (dict(GIST, nprobe=100000), dict(nprobe=4096, wl_stride=3 * 4096, big_nprobe=0)),
    (dict(GIST, nprobe=5, bpl=0), dict(nprobe=5, wl_stride=1)),
    (dict(n_lists=16384, D=960, nq=65, nprobe=8192), dict(nprobe=8192, big_nprobe=0, select="mfma", rank="bf16x3", keywin=0)),
    (dict(n_lists=16384, D=960, nq=65, nprobe=8193), dict(nprobe=8193, big_nprobe=1, select="exact", rank="exact", keywin=1, ksplit=1, prep="wg", lazy=0)),
    (dict(n_lists=16384, D=960, nq=2, nprobe=8193), dict(prep="wg", rank="exact")),  # (no latency front before the exact ranking)
    # top_k: the tie log's capacity at 63 / 64, registers at 256 / 257, the LDS heap at 16384 / 16385
    (dict(GIST, top_k=63), dict(tie=1, tie_cap=2048)),
    (dict(GIST, top_k=64), dict(tie=1, tie_cap=8192)),
    (dict(GIST, top_k=256), dict(tie=1, tie_cap=8192, heap_global=0)),
    (dict(GIST, top_k=257), dict(tie=0, tie_cap=0)),
    (dict(GIST, top_k=16384), dict(heap_global=0)),
    (dict(GIST, top_k=16385), dict(heap_global=1)),
    # ... where scan_lds_bytes crosses 160 KB below kTopKMax: no dimension an index may have (D <= 2048: 30 400 bytes beside the heap)
    # gets there; at D 4096 with 6-bit ex codes 16384 + 17472 + 12800 bytes stand beside it, so 14 648 entries of 8 bytes fit exactly
    (dict(n_lists=4096, D=2048, ex_bits=6, top_k=16384), dict(heap_global=0)),
    (dict(n_lists=4096, D=4096, ex_bits=6, top_k=14647), dict(heap_global=0)),
    (dict(n_lists=4096, D=4096, ex_bits=6, top_k=14648), dict(heap_global=1)),
    # the tie log stays within 1 GiB: 8192 entries of 12 bytes for 10 922 / 10 923 queries
    (dict(GIST, nq=10922, top_k=100, scan_wave=0), dict(tie=1, tie_cap=8192)),
    (dict(GIST, nq=10923, top_k=100, scan_wave=0), dict(tie=0)),
    # D % 64 != 0: the f32 GEMM; D % 16 != 0: no latency kernel either
    (dict(n_lists=4096, D=96, nq=65), dict(rank="f32", prep="wg", ksplit=1, rot_hl=0, tile=64)),
    (dict(n_lists=4096, D=96, nq=2), dict(rank="none", prep="lat_scorers")),
    (dict(n_lists=4096, D=72, nq=2), dict(rank="f32", prep="prep_wave")),
    (dict(n_lists=24576, D=96, nq=128, rank_tile=256), dict(rank="f32", tile=128)),  # (no 256 form of the f32 GEMM)
    # the matrix rotator: k_prep, no latency kernel, no split-K
    (dict(n_lists=24, D=64, rotator=0, nq=1), dict(prep="prep", rank="bf16x3", ksplit=1, tile=64)),
    (dict(GIST, rotator=0, nq=65), dict(prep="prep", rank="bf16x3", ksplit=1)),
    (dict(GIST, rotator=2, nq=65), dict(prep="wg_zero", ksplit=4)),
    # ---- 2. every option that forces a route --------------------------------------------------------------------------------------
    (dict(BIGCALL, rank_tile=64), dict(tile=64, rank="bf16x3")),  # (a forced tile: no f16 by rule)
    (dict(BIGCALL, rank_tile=128, n_lists=4096), dict(tile=128, rank="bf16x3")),
    (dict(BIGCALL, rank_tile=256, n_lists=4096), dict(tile=256, rank="bf16x3", ksplit=1)),
    (dict(BIGCALL, rank_tile=256, rank_f16=1), dict(tile=256, rank="f16")),
    (dict(GIST, nq=65, rank_tile=128), dict(tile=128, ksplit=4, prep="wg_zero")),  # 32 x 1 tiles of 128
    # (a forced 256 tile on a call that asked for parts: the 256 grid has no z — the GEMM runs unsplit on rows the preparation cleared)
    (dict(GIST, nq=65, rank_tile=256), dict(tile=256, ksplit=1, prep="wg_zero", rank="bf16x3")),
    (dict(BIGCALL, rank_f16=0), dict(rank="bf16x3", tile=128)),
    (dict(GIST, nq=600, rank_f16=1), dict(rank="f16", tile=64)),
    (dict(GIST, nq=65, rank_f16=1), dict(rank="bf16x3", ksplit=4)),  # (split-K first)
    (dict(GIST, nq=65, rank_f16=1, rank_ksplit=0), dict(rank="f16", ksplit=1, prep="wg")),
    (dict(GIST, nq=65, rank_ksplit=0), dict(ksplit=1, prep="wg")),
    (dict(GIST, nq=65, rank_ksplit=3), dict(ksplit=3, prep="wg_zero")),
    (dict(GIST, nq=65, rank_ksplit=8), dict(ksplit=4, prep="wg_zero")),
    (dict(GIST, nq=65, D=128, rank_ksplit=3), dict(ksplit=3)),  # (forced: the slab rule does not apply)
    (dict(GIST, nq=600, rank_ksplit=3), dict(ksplit=1, prep="prep_wave")),  # (only behind the workgroup preparation)
    (dict(GIST, nq=65, exact_rank=1), dict(rank="exact", select="exact", ksplit=1, prep="wg", rot_hl=0, lazy=0, keywin=0)),
    (dict(GIST, nq=2, exact_rank=1), dict(rank="exact", prep="wg")),
    (dict(GIST, nq=65, f32_rank=1), dict(rank="f32", ksplit=1, prep="wg", rot_hl=0)),
    (dict(GIST, nq=2, f32_rank=1), dict(rank="f32", prep="wg")),
    (dict(GIST, nq=65, wg_prep=1), dict(prep="prep", ksplit=1, rank="bf16x3")),
    (dict(GIST, nq=2, wg_prep=1), dict(prep="prep", rank="bf16x3")),
    (dict(GIST, nq=600, rank_planar=1), dict(planar=1, planes=1, rank="bf16x3")),
    (dict(GIST, nq=600, rank_planar=1, rank_f16=1), dict(planar=1, rank="bf16x3")),
    (dict(GIST, nq=600, rank_planar=1, probe_installed=1), dict(planar=0, planes=0, rank="bf16x3")),
    (dict(GIST, nq=2, rank_planar=1), dict(planar=0, prep="lat_scorers")),
    (dict(GIST, nq=2, latency_path=0), dict(prep="prep_wave", rank="bf16x3", ksplit=1)),
    (dict(GIST, nq=65, latency_path=0), dict(prep="prep_wave", ksplit=1)),
    (dict(GIST, nq=1000, scan_wave=0), dict(wave=0, tie=1)),
    (dict(GIST, nq=1, scan_wave=1), dict(wave=1, tie=0)),
    (dict(GIST, nq=1000, no_block_bound=1), dict(wave=0, lazy=0)),
    (dict(GIST, nq=65, has_filter=1), dict(lazy=1)),
    (dict(GIST, nq=65, has_filter=1, has_diag=1), dict(lazy=0, tie=0)),
    (dict(GIST, nq=65, has_filter=1, lazy_filter=0), dict(lazy=0)),
    (dict(GIST, nq=65, has_filter=1, head_exact=0), dict(lazy=0)),
    (dict(GIST, nq=65, has_diag=1), dict(lazy=1, tie=0)),
    (dict(GIST, nq=65, lazy_select=0), dict(lazy=0)),
    (dict(GIST, nq=1000, range=1, top_k=100000), dict(lazy=0, wave=0, tie=0, heap_global=0, rank="f16", tile=128)),  # (32 x 8 tiles of 128)
    (dict(GIST, nq=2, stage_mask=0x7), dict(prep="wg", rank="bf16x3", ksplit=1)),  # (a masked call: neither latency front nor split-K)
    (dict(GIST, nq=65, stage_mask=0xd), dict(prep="wg", ksplit=1)),
    (dict(GIST, nq=65, tie_log=0), dict(tie=0)),
    (dict(GIST, nq=65, tie_log_cap=7), dict(tie=1, tie_cap=7)),
    (dict(GIST, nq=65, exact_heap=1), dict(tie=0)),
    (dict(GIST, nq=65, probe_installed=1), dict(tie=0)),
    # the MSTG posting scan: the scan part only, ex codes never evaluated
    (dict(GIST, nq=300, mstg=1, nprobe=77, rotator=2), dict(prep="none", rank="none", wave=1, tie=0, nprobe=77, wl_stride=0, heap_global=0)),
    # (16384 + 16384 + 12800 bytes beside the heap: 14 784 entries fit, where the same index with its ex codes holds 14 648)
    (dict(n_lists=4096, D=4096, ex_bits=6, top_k=14700, mstg=1), dict(heap_global=0)),
    (dict(n_lists=4096, D=4096, ex_bits=6, top_k=14700), dict(heap_global=1)),
    (dict(n_lists=4096, D=4096, ex_bits=6, top_k=14783, mstg=1), dict(heap_global=0)),
    (dict(n_lists=4096, D=4096, ex_bits=6, top_k=14784, mstg=1), dict(heap_global=1)),
]


def test_table_by_hand(plancheck, tmp_path):
    got = run_lines(plancheck, tmp_path, [plan_line(c) for c, _ in TABLE])
    for (case, want), g in zip(TABLE, got):
        assert g["ok"] == "1", (case, g)
        assert same(g, want) is None, (case, same(g, want), g)
        if not case.get("mstg"):
            assert same(g, parent_route(case)) is None, (case, same(g, parent_route(case)))  # (the restatement agrees with the table)


# ---- 3. the sweep -------------------------------------------------------------------------------------------------------------------
def sweep_cases():
    shapes = [dict(n_lists=64, D=64, ex_bits=0), dict(n_lists=4096, D=256, ex_bits=6), dict(n_lists=4096, D=960, ex_bits=6),
              dict(n_lists=24, D=64, rotator=0), dict(n_lists=24576, D=192, ex_bits=2), dict(n_lists=65536, D=960, ex_bits=6),
              dict(n_lists=4096, D=96), dict(n_lists=4096, D=72), dict(n_lists=16384, D=704, rank_f16_ok=0), dict(n_lists=6145, D=1024)]
    nqs = [1, 4, 5, 64, 65, 127, 128, 256, 257, 512, 513, 1024, 2944, 16384]
    calls = [0, 256, 257, 4096]
    tops = [(1, 1), (10, 16), (64, 0), (256, 8192), (257, 8193), (16385, 100000)]  # (top_k, nprobe)
    opts = [dict(), dict(rank_tile=64), dict(rank_tile=128), dict(rank_tile=256), dict(rank_f16=0), dict(rank_f16=1), dict(rank_ksplit=0),
            dict(rank_ksplit=3), dict(rank_ksplit=8), dict(exact_rank=1), dict(f32_rank=1), dict(wg_prep=1), dict(rank_planar=1),
            dict(latency_path=0), dict(scan_wave=0), dict(scan_wave=1), dict(no_block_bound=1), dict(has_filter=1), dict(has_diag=1),
            dict(has_filter=1, has_diag=1), dict(range=1), dict(stage_mask=0x7), dict(stage_mask=0xd), dict(latency_first=1),
            dict(probe_installed=1), dict(rank_tile=256, rank_ksplit=3), dict(rank_tile=256, rank_f16=1), dict(rank_planar=1, rank_f16=1),
            dict(rank_ksplit=3, rank_f16=1), dict(exact_heap=1), dict(tie_log_cap=5)]
    out = []
    for sh, nq, (top_k, nprobe) in itertools.product(shapes, nqs, tops):
        for i, o in enumerate(opts):
            call = calls[(nq + i + top_k) % len(calls)]  # (every call size meets every shape and option, not every triple)
            if call and call < nq:
                call = 0
            out.append(dict(sh, nq=nq, call_nq=call, top_k=top_k, nprobe=nprobe, **o))
    return out


def test_sweep_holds_the_couplings_and_equals_the_parent(plancheck, tmp_path):
    cases = sweep_cases()
    assert len(cases) > 5000
    got = run_lines(plancheck, tmp_path, [plan_line(c) for c in cases])
    seen = set()
    for case, g in zip(cases, got):
        assert g["ok"] == "1", (case, g)
        assert same(g, parent_route(case)) is None, (case, same(g, parent_route(case)))
        seen.add((g["prep"], g["rank"], g["tile"], g["ksplit"], g["select"]))
    # the sweep reaches every form, route, tile and number of parts
    for i, values in enumerate((("prep", "prep_wave", "wg", "wg_zero", "lat_scorers"), ("none", "exact", "f32", "bf16x3", "f16"),
                                ("64", "128", "256"), ("1", "2", "3", "4"), ("exact", "mfma"))):
        assert {s[i] for s in seen} == set(values)


# ---- 4. host_call_plan ----------------------------------------------------------------------------------------------------------------
def test_host_call_plan(plancheck, tmp_path):
    mb = 1 << 20
    # (nq, in_pinned, query_bytes, nsub, host_lanes, host_zero_copy, host_stage_helpers) -> lanes, zero_copy, helpers, latency_first
    table = [
        ((4, 1, mb, 1, 0, 1, 1), (1, 0, 0, 1)),       # up to 4 queries: the latency front would read them over PCIe
        ((5, 1, mb, 1, 0, 1, 1), (1, 1, 0, 1)),
        ((4, 0, mb, 1, 0, 1, 1), (1, 0, 0, 1)),
        ((5, 0, mb, 1, 0, 1, 1), (1, 1, 0, 1)),
        ((1024, 0, 4 * mb, 4, 0, 1, 1), (4, 1, 1, 1)),  # pageable: the window closes at 1024
        ((1025, 0, 4 * mb, 4, 0, 1, 1), (4, 0, 1, 1)),
        ((1025, 1, 4 * mb, 4, 0, 1, 1), (4, 1, 0, 1)),  # page-locked: at 1536
        ((1536, 1, 6 * mb, 4, 0, 1, 1), (4, 1, 0, 1)),
        ((1537, 1, 6 * mb, 4, 0, 1, 1), (4, 0, 0, 1)),
        ((1024, 1, 4 * mb, 4, 0, 0, 1), (4, 0, 0, 1)),  # option host_zero_copy 0
        ((4095, 1, 16 * mb, 4, 0, 1, 1), (4, 0, 0, 1)),  # kHostWaveMinQueries
        ((4096, 1, 16 * mb, 4, 0, 1, 1), (4, 0, 0, 0)),
        ((4096, 0, 16 * mb, 4, 0, 1, 1), (4, 0, 1, 0)),
        ((300, 0, 512 * 1024 - 1, 4, 0, 1, 1), (4, 1, 0, 1)),  # the helpers' floor: 512 KB of queries
        ((300, 0, 512 * 1024, 4, 0, 1, 1), (4, 1, 1, 1)),
        ((300, 1, 512 * 1024, 4, 0, 1, 1), (4, 1, 0, 1)),      # page-locked queries need no staging
        ((300, 0, mb, 4, 0, 1, 0), (4, 1, 0, 1)),              # option host_stage_helpers 0
        ((200, 0, mb, 1, 0, 1, 1), (1, 1, 0, 1)),              # one sub-batch: nothing to help with
        ((8192, 0, 32 * mb, 8, 0, 1, 1), (6, 0, 0, 0)),        # more sub-batches than lanes: lanes are reused, no helpers
        ((8192, 0, 32 * mb, 8, 8, 1, 1), (8, 0, 1, 0)),        # eight lanes: kMaxHelped sub-batches
        ((9216, 0, 36 * mb, 9, 9, 1, 1), (9, 0, 0, 0)),
        ((2048, 0, 8 * mb, 4, 2, 1, 1), (2, 0, 0, 1)),         # option host_lanes 2
    ]
    got = run_lines(plancheck, tmp_path, ["host " + " ".join(str(v) for v in c) for c, _ in table])
    for (case, want), g in zip(table, got):
        assert (int(g["lanes"]), int(g["zero_copy"]), int(g["helpers"]), int(g["latency_first"])) == want, (case, g)
