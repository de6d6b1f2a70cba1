"""Every compile-time instantiation of the two top-k scan kernels against the oracle (`pytest -m gpu`).
k_scanw<DT, EX, TR> and k_scan<DT, EX, TR> exist for DT in {128, 256, 384, 512, 768, 960, 1024, 1536}, EX in {0, 2, 6} (1 / 3 / 7
total bits) and TR in {1, 2, 4} (the registers per lane that hold the top-k), and scanw.hpp / scan.hpp branch `constexpr` on the
triple.  One test per (dim, bits), both metrics, on the cases of tests/scan_instantiation_cases.py (whose fitness the CPU test
tests/test_scan_instantiation_cases_host.py asserts on the oracle alone):
* top_k on both sides of every register-class boundary of both kernels, `_both_kernels` each: ids, counts and diagnostics counters
  exact against the oracle, scores within RTOL, with and without diagnostics, k_scan against k_scanw bit for bit; a filtered call
  (every third id) at top_k 10 and at top_k 100;
* WHICH kernel serves is asserted, not assumed: before the calls of a (dim, bits, top_k) the stage probe (stage_resources, nothing
  is launched) must report k_scanw — 64 threads, at most 16 bytes of scratch — under scan_wave 1 up to top_k 255, and k_scan — 256
  threads — under scan_wave 0 and above 255.  launch_scanw_r declines an instantiation whose code object carries more than 16 bytes
  of scratch, and k_scan then serves with identical results: the instantiations allowed to do so are the literal set DECLINES, which
  equals the rows above 16 bytes of profiles/scan_instantiations/kernel_resources.txt (tools/kernel_resources.sh of this tree).  An
  instantiation outside the set that declines fails the test, and so does a listed one that no longer declines: either the kernel
  changed or the set is stale.
No VGPR figure is asserted: those are the compiler's.  With RBQ_STAGE_RESOURCES_OUT=<file> in the environment every test appends
the scan stage's (threads, vgprs, lds_bytes, scratch_bytes) of its triples, both kernels, to that file as JSON lines
(profiles/scan_instantiations/stage_resources.jsonl is one such run)."""
import json
import os

import pytest

import rabitq_rs_amd as rq
import scan_instantiation_cases as sic
from test_gpu_round5 import _both_kernels

pytestmark = pytest.mark.gpu

K_SCANW_THREADS, K_SCAN_THREADS = 64, 256
K_SCANW_MAX_SCRATCH = 16  # bytes per lane (k_scanw.hip: kScanwMaxScratch)
K_SCANW_MAX_TOP_K = 255   # (k_scanw.hip: scanw_serves)

# (dim, total bits, TR) of the k_scanw instantiations that decline (k_scan serves their calls): k_scanw<960, 6, 4> with 24 bytes
# of scratch and k_scanw<1024, 6, 4> with 40, i.e. 7-bit indexes of dim 960 and 1024 at top_k 128..255
DECLINES = {(960, 7, 4), (1024, 7, 4)}


def scanw_tr(top_k):
    """k_scanw's register class (k_scanw.hip: launch_scanw_t)"""
    return 1 if top_k < 64 else 2 if top_k < 128 else 4


def scan_tr(top_k):
    """k_scan's register class (k_scan.hip: launch_scan_t)"""
    return 2 if 64 <= top_k <= 128 else 4 if 128 < top_k <= 256 else 1


def _served_by(idx, dim, bits, top_k, records):
    """asserts which kernel serves (dim, bits, top_k) under scan_wave 1 and under scan_wave 0; nothing is launched"""
    what = f"dim {dim} bits {bits} top_k {top_k}"
    idx.set_option("scan_wave", 1)
    w = idx.stage_resources(sic.NQ, top_k, sic.NPROBE)["scan"]
    idx.set_option("scan_wave", 0)
    g = idx.stage_resources(sic.NQ, top_k, sic.NPROBE)["scan"]
    idx.set_option("scan_wave", -1)
    for wave, r in ((1, w), (0, g)):
        records.append({"dim": dim, "bits": bits, "top_k": top_k, "scan_wave": wave,
                        "kernel": {K_SCANW_THREADS: "k_scanw", K_SCAN_THREADS: "k_scan"}.get(r["threads"], "?"),
                        "tr": scanw_tr(top_k) if r["threads"] == K_SCANW_THREADS else scan_tr(top_k),
                        "threads": r["threads"], "vgprs": r["vgprs"], "lds_bytes": r["lds_bytes"], "scratch_bytes": r["scratch_bytes"]})
    assert g["threads"] == K_SCAN_THREADS, f"{what}: scan_wave 0 is not served by k_scan: {g}"
    assert w["workgroups"] == sic.NQ and g["workgroups"] == sic.NQ
    if top_k > K_SCANW_MAX_TOP_K:
        assert w["threads"] == K_SCAN_THREADS, f"{what}: above k_scanw's top_k range, yet not served by k_scan: {w}"
    elif (dim, bits, scanw_tr(top_k)) in DECLINES:
        assert w["threads"] == K_SCAN_THREADS, \
            f"{what}: k_scanw<{dim}, {bits - 1}, {scanw_tr(top_k)}> is listed in DECLINES but serves the call ({w}): the list is stale"
    else:
        assert w["threads"] == K_SCANW_THREADS, \
            f"{what}: k_scanw<{dim}, {bits - 1}, {scanw_tr(top_k)}> declined; the kernel that serves instead reports {w['scratch_bytes']} " \
            f"bytes of scratch ({w})"
        assert w["scratch_bytes"] <= K_SCANW_MAX_SCRATCH, f"{what}: k_scanw serves with {w['scratch_bytes']} bytes of scratch"


@pytest.mark.parametrize("bits", sic.BITS)
@pytest.mark.parametrize("dim", sic.DIMS)
def test_every_instantiation_matches_oracle_and_is_the_kernel_that_served(dim, bits):
    records = []
    words, nbits = sic.filter_words()
    try:
        for metric in sic.METRICS:
            _, built, q = sic.case(dim, bits, metric)
            assert built.padded_dim == dim
            idx = rq.IvfRabitqIndex.from_built(built)
            try:
                for top_k in sic.TOP_KS:
                    _served_by(idx, dim, bits, top_k, records if metric == 0 else [])
                    _both_kernels(built, idx, q, top_k, sic.NPROBE)
                for top_k in sic.FILTERED_TOP_KS:
                    _served_by(idx, dim, bits, top_k, records if metric == 0 and top_k not in sic.TOP_KS else [])
                    _both_kernels(built, idx, q, top_k, sic.NPROBE, words, nbits)
            finally:
                idx.close()
    finally:
        out = os.environ.get("RBQ_STAGE_RESOURCES_OUT")
        if out:
            with open(out, "a") as f:
                for r in records:
                    f.write(json.dumps(r) + "\n")


def test_decline_set_is_within_the_sweep():
    """every listed instantiation is one the sweep probes (a stale entry of another dimension could never be found out)"""
    swept = {(d, b, scanw_tr(k)) for d in sic.DIMS for b in sic.BITS for k in sic.TOP_KS + sic.FILTERED_TOP_KS if k <= K_SCANW_MAX_TOP_K}
    assert DECLINES <= swept
    assert {scanw_tr(k) for k in sic.TOP_KS if k <= K_SCANW_MAX_TOP_K} == {1, 2, 4} and {scan_tr(k) for k in sic.TOP_KS} == {1, 2, 4}
