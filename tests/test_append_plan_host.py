"""The host plan of rbq_index_append (csrc/host/rbq_append_plan.hpp) under AddressSanitizer + UBSan: tests/appendcheck_main.cpp is
compiled as a stand-alone program and run as a child process over crafted (old sizes, added counts) vectors; the plan it prints
— new sizes, first blocks, the source block of every new block, the cursors — is compared with a restatement in Python, and no
sanitizer may report anything.  Nothing is loaded into this process."""
import os
import subprocess

import pytest

from conftest import ROOT

U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def appendcheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("appendcheck") / "appendcheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "appendcheck_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def plan_ref(old, add):
    """The plan restated: a list's block j stays its block j, new blocks follow, lists stay in order.  None when refused."""
    nb = lambda n: (n + 31) // 32  # noqa: E731
    new_n, new_gb0, old_gb0, ob, b = [], [], [], 0, 0
    for o, a in zip(old, add):
        n = o + a
        if n > U32:
            return None
        old_gb0.append(ob)
        new_gb0.append(b)
        new_n.append(n)
        ob += nb(o)
        b += nb(n)
        if b * 32 > U32:
            return None
    src = [-2] * b if b <= 65536 else None  # (the program leaves it out above that)
    for c, o in enumerate(old):
        for j in range(nb(new_n[c]) if src is not None else 0):
            src[new_gb0[c] + j] = old_gb0[c] + j if j < nb(o) else -1
    return {"old_blocks": ob, "new_blocks": b, "new_vectors": sum(new_n), "new_n": new_n, "new_gb0": new_gb0, "old_gb0": old_gb0,
            "cursor": list(old), "src": src}


def _parse(line):
    head, *parts = line.split(" | ")
    out = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
    for p in parts:
        name, *vals = p.split()
        out[name] = [int(v) for v in vals]
    return out


CASES = [
    # the geometry edges of the GPU test: empty stays empty, empty gets blocks, untouched partial, partial stays partial, partial
    # fills exactly, partial overflows, 31 + 1, full untouched, full opens a block, 33 + 31 ends on an edge, multi-block
    # untouched, multi-block grows; every later list shifts
    ([0, 0, 1, 5, 5, 5, 31, 32, 32, 33, 64, 100], [0, 40, 0, 3, 27, 60, 1, 0, 1, 31, 0, 70]),
    ([0, 0, 0], [0, 0, 0]),            # empty lists, zero additions
    ([31, 32, 33], [0, 0, 0]),         # zero additions: the identity
    ([31, 32, 33], [1, 1, 1]),
    ([31, 32, 33], [33, 32, 31]),
    ([0, 0, 0, 0], [1, 0, 32, 33]),    # every list empty before
    ([7], [0]),
    ([], []),
    ([1] * 300, [31] * 300),
    ([33] * 50, [0, 1] * 25),
]
BIG = [
    ([4294967200], [0], True),                      # 134217725 full blocks: the largest index
    ([4294967200], [95], False),                    # the list reaches 2^32 - 1: its slots pass 32 bits
    ([4294967200], [96], False),                    # the list would pass 2^32 - 1 vectors
    ([5, 4294967000], [0, 4294967000], False),
    ([2147483616, 2147483584], [0, 33], True),      # 134217727 blocks: the last geometry that fits
    ([2147483616, 2147483584], [0, 65], False),     # one block more: total slots cross 32 bits
    ([2147483616, 2147483584], [1, 64], False),
]


def test_plan_matches_restatement_under_asan_ubsan(appendcheck, tmp_path):
    cases = [(o, a) for o, a in CASES] + [(o, a) for o, a, _ in BIG]
    f = tmp_path / "cases.txt"
    f.write_text("".join(" ".join(map(str, o)) + " | " + " ".join(map(str, a)) + "\n" for o, a in cases))
    out = subprocess.run([appendcheck, str(f)], capture_output=True, text=True, timeout=600)
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (old, add), line in zip(cases, lines):
        want = plan_ref(old, add)
        if want is None:
            assert line.startswith("refused "), (old, add, line[:200])
            continue
        assert line.startswith("ok "), (old, add, line[:200])
        got = _parse(line)
        if want["src"] is None:
            assert "src" not in got and want.pop("src") is None
        assert got == want, (old, add)
    for (old, add, ok), line in zip(BIG, lines[len(CASES):]):
        assert line.startswith("ok ") == ok, (old, add, line[:200])
    assert "32-bit vector slots" in lines[len(CASES) + 1] and "2^32 - 1 vectors" in lines[len(CASES) + 2]
    assert "32-bit vector slots" in lines[len(CASES) + 5]


def test_geometry_edges_case_by_hand(appendcheck, tmp_path):
    """the first case spelt out, so that the restatement above is not the only witness"""
    f = tmp_path / "one.txt"
    f.write_text("0 0 1 5 5 5 31 32 32 33 64 100 | 0 40 0 3 27 60 1 0 1 31 0 70\n")
    out = subprocess.run([appendcheck, str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    got = _parse(out.stdout.splitlines()[0])
    assert got["new_n"] == [0, 40, 1, 8, 32, 65, 32, 32, 33, 64, 64, 170]
    assert got["old_gb0"] == [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11] and got["old_blocks"] == 15
    assert got["new_gb0"] == [0, 0, 2, 3, 4, 5, 8, 9, 10, 12, 14, 16] and got["new_blocks"] == 22
    assert got["cursor"] == [0, 0, 1, 5, 5, 5, 31, 32, 32, 33, 64, 100]
    assert got["src"] == [-1, -1, 0, 1, 2, 3, -1, -1, 4, 5, 6, -1, 7, 8, 9, 10, 11, 12, 13, 14, -1, -1]
    assert got["new_vectors"] == 541
