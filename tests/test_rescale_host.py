"""The per-vector rescale factor of RabitqConfig::new (best_rescale_factor, reference src/quantizer.rs:337-427), the parts
that need no GPU: the CPU builder's export against a plain-Python heapq restatement, bit for bit, on crafted inputs; and
the compiled k_rescale unit (the device search) uses no scratch."""
import glob
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import ROOT
from rescale_ref import best_rescale_factor, crafted_rows, normalize


def _bits(x):
    return struct.pack("<d", x).hex()


@pytest.mark.parametrize("ex_bits", [2, 6])
@pytest.mark.parametrize("dim", [64, 128, 960, 2048])
def test_cpu_best_rescale_factor_matches_heapq_restatement(dim, ex_bits):
    for name, o in crafted_rows(dim, 1000 * dim + ex_bits):
        want = best_rescale_factor(o, ex_bits)
        got = rq.builder.best_rescale_factor(o, ex_bits)
        assert _bits(got) == _bits(want), (name, got, want)
    rng = np.random.default_rng(dim + ex_bits)
    for _ in range(8):
        o = normalize(rng.standard_normal(dim))
        assert _bits(rq.builder.best_rescale_factor(o, ex_bits)) == _bits(best_rescale_factor(o, ex_bits))


@pytest.mark.parametrize("ex_bits", [1, 3, 4, 5, 7])
def test_cpu_best_rescale_factor_other_widths(ex_bits):
    """ex 1: the start code of the largest coordinate is already 2^ex - 1, its first event still counts."""
    for name, o in crafted_rows(96, 7 + ex_bits):
        assert _bits(rq.builder.best_rescale_factor(o, ex_bits)) == _bits(best_rescale_factor(o, ex_bits)), name


def test_restatement_self_checks():
    o = normalize(np.ones(64))
    assert best_rescale_factor(np.zeros(64, np.float32), 6) == 1.0
    t = best_rescale_factor(o, 6)
    # a constant vector codes every coordinate alike: t lands on an event k / o for a whole k
    k = t * float(o[0])
    assert abs(k - round(k)) < 1e-9 and 1 <= round(k) <= 63
    # the peaked row's largest coordinate reaches the top code at t
    _, p = crafted_rows(64, 3)[7]
    tp = best_rescale_factor(p, 2)
    assert int(tp * float(p.max()) + 1e-5) >= 3


def test_k_rescale_uses_no_scratch(tmp_path):
    """k_rescale.hip compiled with the product flags: private_segment_fixed_size 0 (all per-coordinate state in LDS), and
    the f64 division / square root are the IEEE sequences (v_div_fixup_f64), not approximations."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rabitq-rs_amd", "csrc", "device", "k_rescale.hip")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-gpu-rdc",
                           "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "--save-temps", "-c", src, "-o",
                           str(tmp_path / "k_rescale.o")], cwd=str(tmp_path), stderr=subprocess.DEVNULL)
    asm = open(glob.glob(str(tmp_path / "*gfx950*.s"))[0]).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN3rbq\w*k_rescale\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S)}
    assert len(bodies) == 1, sorted(bodies)
    body = next(iter(bodies.values()))
    assert not re.findall(r"^\s+(scratch_\w+|buffer_store\w*)", body, flags=re.M)
    assert "v_div_fixup_f64" in body
    sizes = re.findall(r"\.name:\s+(_ZN3rbq\S*k_rescale\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm)
    assert sizes and all(int(s) == 0 for _, s in sizes), sizes
