"""The layout of the ranking GEMM's split-bf16 operand images (csrc/device/hl_layout.hpp, hl_offset) without a GPU: a
small program around the one mapping that the writing kernels, the GEMM's strides and the host mirror of the debug copies share
prints the offset of every (element, plane) of a row; the mapping must be a bijection onto [0, 2 D), and both planes of K slab s
must lie in the aligned 128-byte unit s of the row, hi first."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DIMS = [64, 128, 960, 1024]
SLAB = 32  # elements of a K slab: 64 bytes of bf16 per plane

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "hl_layout.hpp"
int main(int argc, char** argv) {
    const uint32_t D = (uint32_t)std::atoi(argv[1]);
    std::printf("%u\n", rbq::kHlSlab);
    for (uint32_t plane = 0; plane < 2; ++plane)
        for (uint32_t i = 0; i < D; ++i) std::printf("%u\n", rbq::hl_offset(i, plane, D));
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_lines")
    src, out = str(d / "hl_main.cpp"), str(d / "hl_main")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "device"), "-o", out, src])
    return out


def _offsets(exe, D):
    out = subprocess.run([exe, str(D)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    v = np.array(out, dtype=np.int64)
    assert v.size == 1 + 2 * D
    return int(v[0]), v[1:].reshape(2, D)  # [plane][element]


@pytest.mark.parametrize("D", DIMS)
def test_mapping_is_a_bijection(exe, D):
    slab, off = _offsets(exe, D)
    assert slab == SLAB
    assert np.array_equal(np.sort(off.ravel()), np.arange(2 * D)), "not a bijection onto [0, 2 D)"


@pytest.mark.parametrize("D", DIMS)
def test_both_planes_of_a_slab_share_one_line(exe, D):
    _, off = _offsets(exe, D)
    i = np.arange(D)
    s = i // SLAB
    byte = off * 2  # bf16 elements
    for plane in (0, 1):
        assert np.array_equal(byte[plane] // 128, s), f"plane {plane}: an element of slab s outside the 128-byte unit s"
        # hi in the first 64 bytes of the line, lo in the last 64, the elements of a plane in order
        assert np.array_equal(byte[plane] % 128, 64 * plane + 2 * (i % SLAB))
    # the strides the GEMM is launched with: rows of 4 D bytes, slabs of 128, the lo plane 64 bytes behind the hi plane
    assert np.array_equal(byte[1] - byte[0], np.full(D, 64))
    assert int(byte.max()) + 2 == 4 * D


def interleave(hi, lo):
    """numpy restatement for D % 32 == 0: [rows][D] planes -> [rows][2 D] image, per K slab the 32 hi then the 32 lo values."""
    r, D = hi.shape
    assert D % SLAB == 0 and lo.shape == hi.shape
    return np.concatenate([hi.reshape(r, D // SLAB, SLAB), lo.reshape(r, D // SLAB, SLAB)], axis=2).reshape(r, 2 * D)


@pytest.mark.parametrize("D", DIMS)
def test_numpy_restatement_matches(exe, D):
    """The numpy interleave that tests/test_gpu_rank_lines.py compares the device images with is this mapping."""
    _, off = _offsets(exe, D)
    hi = np.arange(3 * D, dtype=np.uint16).reshape(3, D)
    lo = hi + np.uint16(30000)
    img = interleave(hi, lo)
    assert img.shape == (3, 2 * D)
    assert np.array_equal(img[:, off[0]], hi) and np.array_equal(img[:, off[1]], lo)
