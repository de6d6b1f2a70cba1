"""The GPU-free half of rbq_index_load_rbq1_stream (csrc/host/rbq_load_stream.hpp: framing pass, span cutter, the prefix check
as a plain loop, verdict) against rbq1_parse, under AddressSanitizer + UBSan.  tests/loadcheck_main.cpp is compiled as a
stand-alone program and run as a child process over the error corpus of tests/load_stream_cases.py, at the smallest span and
at an odd one: both answers must agree for every stream, the spans' pieces must tile the cluster region exactly once, and no
sanitizer may report anything.  Nothing is loaded into this process."""
import os
import subprocess

import pytest

import load_stream_cases as cases
from conftest import ROOT


@pytest.fixture(scope="module")
def loadcheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loadcheck") / "loadcheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "loadcheck_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe, tmp_path, named, spans):
    paths = []
    for i, (_, data) in enumerate(named):
        p = tmp_path / f"s{i:04d}.rbq"
        p.write_bytes(data)
        paths.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    out = subprocess.run([exe, str(lst)] + [str(s) for s in spans], capture_output=True, text=True, timeout=600)
    lines = out.stdout.splitlines()
    return out, lines


# the smallest span (one 640-byte batch record; 1 is raised to it), an odd one of a few units, the default
SPANS = (1, 2333, 0)


def test_corpus_agrees_with_rbq1_parse_under_asan_ubsan(loadcheck, tmp_path):
    named = cases.corpus(cases.base_stream())
    out, lines = _run(loadcheck, tmp_path, named, SPANS)
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert len(lines) == len(named) * len(SPANS), (out.stdout[-2000:], out.stderr[-2000:])
    bad = [(named[i // len(SPANS)][0], ln.split(" span=", 1)[1]) for i, ln in enumerate(lines) if not ln.endswith("| AGREE")]
    assert not bad, bad[:10]
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr[-4000:]
    # the corpus is not all one answer: every message of rbq1_parse that the issue's cases aim at shows up
    seen = {ln.split(" | parse rc=", 1)[1].split(" | lists=", 1)[0] for ln in lines}
    for want in ("0 detail=", "failed to fill whole buffer", "unrecognized file header", "unsupported index format version",
                 "dimension must be positive", "padded_dim must be >= dim", "unknown metric tag", "unknown rotator type tag",
                 "ex_bits out of range", "total_bits out of range", "total_bits does not match ex_bits",
                 "FHT rotator flip bits length mismatch", "cluster size exceeds reasonable limits", "batch_data length mismatch",
                 "ex_code_packed length mismatch", "vector count metadata mismatch", "checksum mismatch"):
        assert any(want in s for s in seen), want


def test_good_streams_of_every_shape_tile_and_agree(loadcheck, tmp_path):
    """self-consistent random streams: odd list sizes, 1-, 3- and 7-bit, a dimension whose record exceeds the odd span"""
    named = []
    for ex_bits, sizes, d in ((0, [0, 1, 31, 32, 33, 300, 0, 65], 64), (2, [0, 1, 31, 32, 33, 300, 0, 65], 128),
                              (6, [5, 0, 0, 70], 2048), (6, [], 64), (2, [0, 0, 0], 64), (6, [1], 960)):
        named.append((f"ex{ex_bits}-d{d}-{sizes}", cases._random_stream(ex_bits, sizes, d=d, seed=ex_bits + d)))
    out, lines = _run(loadcheck, tmp_path, named, SPANS + (8576 * 3 + 4,))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.returncode == 0 and not out.stderr.strip(), (out.stdout[-2000:], out.stderr[-4000:])
    assert len(lines) == len(named) * 4 and all(ln.endswith("| AGREE") and " parse rc=0 " in ln for ln in lines)
