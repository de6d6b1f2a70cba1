"""The plan of a brute-force call (rbq_host::plan_bf_call, csrc/host/rbq_bf_plan.hpp): vectors per chunk, chunks, queries per
sub-batch and what the call's own buffers are sized by, checked without a GPU: a stand-alone program under AddressSanitizer +
UBSan (tests/bfplancheck_main.cpp) prints the plan of every case — nothing sanitized is loaded into this process.

Expected values come from two sources that do not read the header: the launch counts test_gpu_bf_chunks.py spells out by hand
(launches = sub-batches x chunks), and `parent_topk` / `parent_range`, the formulas as bf_search_impl and bf_range_impl wrote
them out, each for itself, before the plan existed."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

DIST_BUDGET, HEAP_BUDGET, OUT_BUDGET, MAX_SUB, LDS_HEAP_MAX_TOP_K, RANGE_SPAN = 128 << 20, 48 << 20, 48 << 20, 1024, 8191, 2048
U32, U64 = 2 ** 32 - 1, 2 ** 64 - 1


@pytest.fixture(scope="module")
def bfplancheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bfplancheck") / "bfplancheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "bfplancheck_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def plans(exe, tmp_path, cases):
    """the plan of every (n, nq, range, top_k or capacity, chunk cap), as a dict of ints"""
    path = tmp_path / "cases.txt"
    path.write_text("".join("%d %d %d %d %d\n" % c for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(cases)
    return [{k: int(v) for k, v in (tok.split("=") for tok in r.split())} for r in rows]


def _ceil(a, b):
    return -(-a // b)


# ---- the parent's two formulas, restated from bf_search_impl and bf_range_impl as they stood --------------------------------------
def parent_topk(n, nq, top_k, cap):
    nv_chunk = min(n, DIST_BUDGET // 4, cap if cap else U64)
    n_chunks = (n + nv_chunk - 1) // nv_chunk
    lds_heap = top_k <= LDS_HEAP_MAX_TOP_K
    heap_ws = n_chunks > 1 or not lds_heap
    sub = min(nq, MAX_SUB, max(1, DIST_BUDGET // (nv_chunk * 4)), max(1, OUT_BUDGET // (top_k * 12)))
    if heap_ws:
        sub = min(sub, max(1, HEAP_BUDGET // ((top_k + 1) * 8)))
    return dict(nv_chunk=nv_chunk, n_chunks=n_chunks, sub=sub, lds_heap=int(lds_heap), heap_ws=int(heap_ws), cap=0, spans=0)


def parent_range(n, nq, capacity, limit):
    nv_chunk = min(n, DIST_BUDGET // 4, limit if limit else U64)
    n_chunks = (n + nv_chunk - 1) // nv_chunk
    spans = (nv_chunk + RANGE_SPAN - 1) // RANGE_SPAN
    cap = min(capacity, n)
    sub = min(nq, MAX_SUB, max(1, DIST_BUDGET // (nv_chunk * 4)))
    if cap:
        sub = min(sub, max(1, OUT_BUDGET // (cap * 12)))
    return dict(nv_chunk=nv_chunk, n_chunks=n_chunks, sub=sub, lds_heap=0, heap_ws=0, cap=cap, spans=spans)


# ---- 1. the launch counts spelt out by hand in test_gpu_bf_chunks.py::test_launch_plan_of_the_cases_below --------------------------
LAUNCHES = [((700, 9, 10, c), want) for c, want in zip((0, 64, 65, 511, 512, 513, 699, 700, 701), (1, 11, 11, 2, 2, 2, 2, 1, 1))] + [
    ((500, 7, 10, 96), 6), ((1200, 4, 20, 100), 12), ((2000, 20, 100, 333), 7),
    ((20000, 3, 16384, 0), 1), ((20000, 3, 8191, 4096), 5), ((10000, 3, 9000, 4096), 3),
    ((40, 257, 16384, 0), 2), ((40, 257, 16384, 16), 6), ((5000, 200, 10, 1024), 5)]


def test_launch_counts_by_hand(bfplancheck, tmp_path):
    got = plans(bfplancheck, tmp_path, [(n, nq, 0, k, cap) for (n, nq, k, cap), _ in LAUNCHES])
    for ((n, nq, k, cap), want), p in zip(LAUNCHES, got):
        assert _ceil(nq, p["sub"]) * p["n_chunks"] == want, ((n, nq, k, cap), p)
        assert p == parent_topk(n, nq, k, cap), ((n, nq, k, cap), p)  # (the restatement agrees with the table)


# ---- 2. the grid: every min and max of the formulas is crossed ---------------------------------------------------------------------
NS = (1, 40, 700, 8191, 8192, 2 ** 25, 2 ** 25 + 1, U32)  # 2^25 = kBfDistBudget / 4
NQS = (1, 257, 1024, 1025)
TOP_KS = (1, 8191, 8192, 16384)


def grid():
    out = []
    for n, nq in itertools.product(NS, NQS):
        for limit in sorted({0, 1, 64, n, n + 1}):
            out += [(n, nq, 0, k, limit) for k in TOP_KS]
            # (the capacity is a uint32_t of the C entry: n + 1 of the largest n does not exist)
            out += [(n, nq, 1, c, limit) for c in sorted({0, 1, n - 1, n, n + 1, 2 ** 20}) if c <= U32]
    return out


def test_grid_equals_the_parent(bfplancheck, tmp_path):
    cases = grid()
    assert len(cases) > 1400
    got = plans(bfplancheck, tmp_path, cases)
    seen = set()
    for (n, nq, rng, k, limit), p in zip(cases, got):
        want = parent_range(n, nq, k, limit) if rng else parent_topk(n, nq, k, limit)
        assert p == want, ((n, nq, rng, k, limit), p, want)
        # what the loops of the call divide and step by
        assert p["sub"] >= 1 and p["nv_chunk"] >= 1 and p["n_chunks"] * p["nv_chunk"] >= n, ((n, nq, rng, k, limit), p)
        assert (p["n_chunks"] - 1) * p["nv_chunk"] < n  # (no empty chunk)
        seen.add((rng, p["n_chunks"] > 1, p["sub"] < min(nq, MAX_SUB), p["lds_heap"], p["heap_ws"], p["cap"] < k))
    # both kinds with one and with several chunks, sub-batches cut by a budget, every heap form, a capacity above n
    assert {s[:3] for s in seen} == set(itertools.product((0, 1), (False, True), (False, True)))
    assert {s[3:5] for s in seen if not s[0]} == {(1, 0), (1, 1), (0, 1)}
    assert any(s[0] and s[5] for s in seen)
