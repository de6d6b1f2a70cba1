"""The exact MSTG range search (options "mstg_range_exact" / "mstg_range_exact_bits") without a GPU: the
restatement tests/mstg_range_exact_ref.py against a direct NumPy pass, the option names in rbq.h's list, and the refusal texts of
rbq_host::mstg_range_exact_check through a stand-alone program (tests/mstg_range_exact_check_main.cpp) run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import mstg_range_exact_ref as xref
import mstg_range_ref as rref
import mstg_rerank_ref as kref
from rabitq_rs_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("metric", [0, 1])
def test_restatement_equals_a_direct_pass(metric):
    # r = +inf: the matches are the distinct ids of ALL candidates with exact distance < x, each at the scan rank of its smallest estimate
    case, q = rref.main_case(metric, 64)
    cands = rref.estimates(case, q, 48, 0.6)[2]
    x = xref.kth_exact_radius(cands, q, case.x, metric, np.inf, 20)
    ids, bits, cnt, ncand = xref.exact_rows(cands, q, case.x, metric, np.inf, x, 64)
    assert cnt[-1] == rref.U32_MAX and (ids[-1] == rref.NONE64).all()  # the far query exceeds the limit: passed through
    assert ((cnt[:-1] > 0) & (cnt[:-1] < ncand[:-1])).any() and (cnt[:-1] > 64).any()
    for i, (cid, est) in enumerate(cands[:-1]):
        uniq = np.unique(cid)
        d = kref.distances(q[i], case.x, uniq, metric)
        k = min(int(cnt[i]), 64)
        assert cnt[i] == (d < x).sum() and np.isin(ids[i, :k], uniq[d < x]).all() and len(set(ids[i, :k].tolist())) == k
        assert np.array_equal(bits[i, :k], d[np.searchsorted(uniq, ids[i, :k])].view(np.uint32)) and (ids[i, k:] == rref.NONE64).all()
        rank = [int(np.nonzero((cid == v) & (est == est[cid == v].min()))[0][0]) for v in ids[i, :k]]  # the smallest estimate's first entry
        assert rank == sorted(rank)
    assert not xref.exact_rows(cands[:-1], q, case.x, metric, np.inf, np.nan, 4)[2].any()


def test_option_names_are_in_the_option_list():
    rbq_h = open(os.path.join(ROOT, "include", "rbq.h")).read()
    listed = rbq_h[rbq_h.index('"rerank_pool" v'):rbq_h.index("int rbq_debug_set_option(")]
    assert '"mstg_range_exact" 0/1' in listed and '"mstg_range_exact_bits" v' in listed
    assert '"mstg_range_exact"' in open(os.path.join(ROOT, "include", "ext", "rbq_mstg_range.h")).read()


def test_refusal_for_all_sixteen_combinations(tmp_path):
    exe = str(tmp_path / "mstg_range_exact_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "mstg_range_exact_check_main.cpp"), "-o", exe]
    for c in (cmd, [exe]):
        out = subprocess.run(c, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
    rows = [r.split(" ", 5) for r in out.stdout.splitlines()]
    assert sorted(tuple(map(int, r[:4])) for r in rows) == [(m >> 3, m >> 2 & 1, m >> 1 & 1, m & 1) for m in range(16)]
    for *flags, rc, detail in rows:
        option, distinct, have_raw, rerank_on = map(int, flags)
        if not option or (distinct and have_raw and rerank_on):
            assert int(rc) == _abi.RBQ_OK and detail == ""
            continue
        way_out = "distinct 1" if not distinct else "raw vectors attached" if not have_raw else "rerank 1"  # the first that applies
        assert int(rc) == _abi.RBQ_INVALID_CONFIG and way_out in detail and "mstg_range_exact 0" in detail, (flags, detail)
