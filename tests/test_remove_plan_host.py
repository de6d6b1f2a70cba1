"""The host plan of rbq_index_remove_ids (csrc/host/rbq_remove_plan.hpp) under AddressSanitizer + UBSan: tests/removecheck_main.cpp
is compiled as a stand-alone program and run as a child process over crafted (old sizes, removed positions) and (old sizes, kept
counts) vectors; the plan it prints — new sizes, first blocks, the source slot of every new slot — is compared with a restatement
in Python and with one case spelt out by hand, and no sanitizer may report anything.  Nothing is loaded into this process."""
import os
import subprocess

import pytest

from conftest import ROOT

U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def removecheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("removecheck") / "removecheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "removecheck_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def plan_ref(old, kept):
    """The plan restated: lists stay in order, a list takes ceil(n / 32) blocks.  None when refused."""
    nb = lambda n: (n + 31) // 32  # noqa: E731
    new_gb0, old_gb0, ob, b = [], [], 0, 0
    for o, k in zip(old, kept):
        if k > o:
            return None
        old_gb0.append(ob)
        new_gb0.append(b)
        ob += nb(o)
        b += nb(k)
        if ob * 32 > U32 or b * 32 > U32:
            return None
    return {"old_blocks": ob, "new_blocks": b, "old_vectors": sum(old), "new_vectors": sum(kept), "new_n": list(kept),
            "new_gb0": new_gb0, "old_gb0": old_gb0}


def map_ref(old, removed):
    """(kept counts, slot map) restated without masks or scans: the survivors of every list in order, 32 to a block"""
    gone, kept, smap, base, ob = set(removed), [], [], 0, 0
    for o in old:
        stay = [ob * 32 + q for q in range(o) if base + q not in gone]
        kept.append(len(stay))
        smap += stay + [-1] * (-len(stay) % 32)
        base += o
        ob += (o + 31) // 32
    return kept, smap


def _parse(line):
    head, *parts = line.split(" | ")
    out = {k: int(v) for k, v in (kv.split("=") for kv in head.split()[1:])}
    for p in parts:
        name, *vals = p.split()
        out[name] = [int(v) for v in vals]
    return out


def _positions(old, per_list):
    """global positions from per-list positions"""
    out, base = [], 0
    for o, pos in zip(old, per_list):
        out += [base + q for q in pos]
        base += o
    return out


# the geometry edges of the GPU test (tests/test_gpu_remove.py), list by list
GEO_OLD = [0, 1, 1, 5, 5, 31, 32, 32, 33, 33, 64, 64, 100, 100, 100, 70]
GEO_POS = [[], [], [0], [0], [4], [], [7], list(range(32)), [32], [0], list(range(0, 64, 2)), list(range(32)), [31, 32, 57],
           [q for q in range(100) if q % 13 and q % 7 != 3 and q != 99][:69], list(range(100)), []]
P_CASES = [
    (GEO_OLD, _positions(GEO_OLD, GEO_POS)),
    ([0, 0, 0], []),                                   # all-empty lists
    ([], []),                                          # zero lists
    ([7], []),                                         # nothing removed: the identity
    ([7], list(range(7))),                             # everything removed
    ([31, 32, 33], [30, 31, 63, 95]),                  # the last of each list (and the first of the second)
    ([31, 32, 33], list(range(96))),
    ([33] * 50, list(range(0, 33 * 50, 33))),          # lane 0 of every list: every list loses its tail block
    ([1] * 300, list(range(0, 300, 2))),               # every second list empties
    ([64, 64], list(range(32)) + list(range(96, 128))),
    ([100], [5, 5, 5]),                                # a position given more than once
]
K_CASES = [
    ([4294967200], [4294967200], True),                 # 134217725 full blocks: the largest index, nothing removed
    ([4294967200], [0], True),                          # ... and emptied
    ([4294967265], [0], False),                         # 134217728 old blocks: the old index passes 2^32 slots
    ([4294967295], [5], False),
    ([2147483616, 2147483648], [2147483616, 31], True),   # 134217727 old blocks: the last geometry that fits
    ([2147483616, 2147483649], [0, 0], False),          # one block more
    ([5, 9], [6, 9], False),                            # a list cannot keep more than it holds
    ([5, 9], [5, 10], False),
    ([5, 9], [0, 0], True),
]


def test_plan_and_slot_map_match_restatement_under_asan_ubsan(removecheck, tmp_path):
    f = tmp_path / "cases.txt"
    f.write_text("".join("P " + " ".join(map(str, o)) + " | " + " ".join(map(str, r)) + "\n" for o, r in P_CASES) +
                 "".join("K " + " ".join(map(str, o)) + " | " + " ".join(map(str, k)) + "\n" for o, k, _ in K_CASES))
    out = subprocess.run([removecheck, str(f)], capture_output=True, text=True, timeout=600)
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(P_CASES) + len(K_CASES)
    for (old, removed), line in zip(P_CASES, lines):
        kept, smap = map_ref(old, removed)
        want = plan_ref(old, kept)
        assert line.startswith("ok "), (old, line[:200])
        want["map"] = smap
        assert _parse(line) == want, (old, removed)
    for (old, kept, ok), line in zip(K_CASES, lines[len(P_CASES):]):
        want = plan_ref(old, kept)
        assert (want is not None) == ok and line.startswith("ok ") == ok, (old, kept, line[:200])
        if ok:
            assert _parse(line) == want, (old, kept)
    k0 = len(P_CASES)
    assert "32-bit vector slots" in lines[k0 + 2] and "32-bit vector slots" in lines[k0 + 3] and "32-bit vector slots" in lines[k0 + 5]
    assert "list 0 would keep more" in lines[k0 + 6] and "list 1 would keep more" in lines[k0 + 7]


def test_small_case_by_hand(removecheck, tmp_path):
    """one case spelt out, so that the restatement above is not the only witness: lists of 3, 33, 0 and 34 vectors; removed are
    the middle one of list 0, lanes 0 and 32 of list 1 and everything but lane 33 of list 3"""
    f = tmp_path / "one.txt"
    pos = [1, 3, 35] + [36 + q for q in range(34) if q != 33]
    f.write_text("P 3 33 0 34 | " + " ".join(map(str, pos)) + "\n")
    out = subprocess.run([removecheck, str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    got = _parse(out.stdout.splitlines()[0])
    assert got["new_n"] == [2, 31, 0, 1]
    assert got["old_gb0"] == [0, 1, 3, 3] and got["old_blocks"] == 5 and got["old_vectors"] == 70
    assert got["new_gb0"] == [0, 1, 2, 2] and got["new_blocks"] == 3 and got["new_vectors"] == 34
    # list 0 (old block 0): slots 0 and 2 stay; list 1 (old blocks 1, 2): slots 33 .. 63 stay, its 33rd vector (slot 64) goes;
    # list 3 (old blocks 3, 4): only lane 1 of its second block (slot 129) stays
    assert got["map"] == [0, 2] + [-1] * 30 + list(range(33, 64)) + [-1] + [129] + [-1] * 31
