"""The layout of a replica's device arrays (csrc/host/rbq_index_layout.hpp) under AddressSanitizer + UBSan:
tests/indexlayout_main.cpp is compiled as a stand-alone program and run as a child process over crafted list sizes and
(D, Dc, ex_bits); what it prints — first blocks, totals, the block tables, the descending prefix sums, every byte size — is
compared with a restatement in Python, and no sanitizer may report anything.  Nothing is loaded into this process."""
import os
import subprocess

import pytest

from conftest import ROOT

U32 = 0xFFFFFFFF
DIMS = [(16, 64, 0), (64, 64, 2), (96, 128, 6), (960, 960, 6), (2048, 2048, 2)]
SMALL = [[], [0], [0, 0, 0], [1], [31], [32], [33], [0, 1, 31, 32, 33, 64, 65, 5], [1] * 300]
# (list sizes as the program reads them, the sizes expanded, accepted?)
BIG = [
    ("4294967295", [U32], False),                                  # one list of 2^32 - 1: 2^27 blocks, 2^32 slots
    ("4294967264", [2**32 - 32], True),                            # 2^27 - 1 full blocks in one list: the largest index
    ("4294967264 1", [2**32 - 32, 1], False),                      # one block later
    ("4095*1048576 1048544", [1 << 20] * 4095 + [(1 << 20) - 32], True),     # 2^27 - 1 blocks over 4096 lists: slots = 2^32 - 32
    ("4095*1048576 1048544 1", [1 << 20] * 4095 + [(1 << 20) - 32, 1], False),  # one block later: slots = 2^32
    ("4095*1048576 1048513 0 0", [1 << 20] * 4095 + [(1 << 20) - 63, 0, 0], True),  # a partly filled last block, empty lists after it
]


@pytest.fixture(scope="module")
def indexlayout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("indexlayout") / "indexlayout")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "indexlayout_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def layout_ref(ln, D, Dc, ex):
    """The layout restated.  None when refused."""
    nb = [(n + 31) // 32 for n in ln]
    gb0, b = [], 0
    for k in nb:
        gb0.append(b)
        b += k
        if b * 32 > U32:
            return None
    out = {"blocks": b, "vectors": sum(ln), "gb0": gb0, "prefix": [0]}
    for k in sorted(nb, reverse=True):
        out["prefix"].append(out["prefix"][-1] + k)
    if b <= 65536:  # (the program leaves the block tables out above that)
        out["block_list"] = [c for c, k in enumerate(nb) for _ in range(k)]
        out["block_nv"] = [min(32, n - 32 * j) for n, k in zip(ln, nb) for j in range(k)]
    codes_per_unit = 128 // ex if ex else 1                               # ex codes in one 16-byte unit, none straddling
    ex_slot = -(-(D // 16) // codes_per_unit) * 16 * 16 if ex else 0      # units per lane x 16 lanes x 16 bytes
    slots, nl = b * 32, len(ln)
    out["bytes"] = {
        "block_stride": Dc * 32 // 8 + 3 * 32 * 4, "ex_slot": ex_slot, "slots": slots, "blocks": b * (Dc * 4 + 384), "ids": slots * 8,
        "ex": slots * ex_slot, "ex_alloc": slots * ex_slot + 256 if ex else 0, "fadd_ex": slots * 4 if ex else 0,
        "fres_ex": slots * 4 if ex else 0, "bsum": b * 32, "bsumx": b * 32, "lsum": nl * 32, "delta": slots * 4, "vl": slots * 4,
        "rnorm": slots * 4, "centroids": nl * D * 4, "cent_hl": nl * D * 2 * 2, "cent_f16": nl * D * 2, "cent_f16_resid": nl * 4,
        "cnorm2": nl * 4, "list_gb0": nl * 4, "list_n": nl * 4}
    return out


def _parse(line):
    head, *parts = line.split(" | ")
    out = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
    for p in parts:
        name, *vals = p.split()
        out[name] = {k: int(v) for k, v in (kv.split("=") for kv in vals)} if name == "bytes" else [int(v) for v in vals]
    return out


def test_layout_matches_restatement_under_asan_ubsan(indexlayout, tmp_path):
    cases = [(" ".join(map(str, ln)), ln, True) for ln in SMALL] + BIG
    runs = [(text, ln, ok, dims) for text, ln, ok in cases for dims in DIMS]
    f = tmp_path / "cases.txt"
    f.write_text("".join("%d %d %d | %s\n" % (*dims, text) for text, _, _, dims in runs))
    out = subprocess.run([indexlayout, str(f)], capture_output=True, text=True, timeout=600)
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(runs)
    for (text, ln, ok, dims), line in zip(runs, lines):
        want = layout_ref(ln, *dims)
        assert (want is not None) == ok, (text, "the restatement disagrees with the case's own verdict")
        if not ok:
            assert line == "refused index too large for 32-bit vector slots", (text, line[:200])
            continue
        assert line.startswith("ok "), (text, dims, line[:200])
        assert _parse(line) == want, (text, dims)


def test_edge_sizes_by_hand(indexlayout, tmp_path):
    """one case spelt out, so that the restatement above is not the only witness"""
    f = tmp_path / "one.txt"
    f.write_text("96 128 6 | 0 1 31 32 33 64 65 5\n64 64 0 | 4095*1048576 1048544\n")
    out = subprocess.run([indexlayout, str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    a, b = (_parse(line) for line in out.stdout.splitlines())
    assert a["gb0"] == [0, 0, 1, 2, 3, 5, 7, 10] and a["blocks"] == 11 and a["vectors"] == 231
    assert a["block_list"] == [1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 7]
    assert a["block_nv"] == [1, 31, 32, 32, 1, 32, 32, 32, 32, 1, 5]
    assert a["prefix"] == [0, 3, 5, 7, 8, 9, 10, 11, 11]
    y = a["bytes"]
    assert y["block_stride"] == 896 and y["ex_slot"] == 256 and y["slots"] == 352 and y["blocks"] == 9856 and y["ids"] == 2816
    assert y["ex"] == 90112 and y["ex_alloc"] == 90368 and y["fadd_ex"] == y["fres_ex"] == y["delta"] == y["vl"] == y["rnorm"] == 1408
    assert y["bsum"] == y["bsumx"] == 352 and y["lsum"] == 256 and y["centroids"] == y["cent_hl"] == 3072 and y["cent_f16"] == 1536
    assert y["cent_f16_resid"] == y["cnorm2"] == y["list_gb0"] == y["list_n"] == 32
    assert b["blocks"] == 2**27 - 1 and b["bytes"]["slots"] == 2**32 - 32 and b["vectors"] == 2**32 - 32 and "block_list" not in b
    assert b["bytes"]["ex"] == 0 and b["bytes"]["ex_alloc"] == 0 and b["bytes"]["blocks"] == (2**27 - 1) * 640
