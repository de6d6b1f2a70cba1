"""The exact rerank of the MSTG candidate pool (option "mstg_rerank") without a GPU: the NumPy restatement
tests/mstg_rerank_ref.py is anchored to a brute-force argsort of the canonical distances, the data of the GPU test is shown to
have no estimate tie at a pool's cut, the recall theorem is checked, and the refusal — a pure function of
csrc/host/rbq_host_logic.hpp — is printed by a stand-alone program built with AddressSanitizer + UBSan
(tests/mstg_rerank_check_main.cpp) and run as a child process: nothing sanitized is loaded into this process."""
import os
import re
import subprocess

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import ROOT
from rabitq_rs_amd import _abi
import mstg_refine_ref as rref
import mstg_rerank_ref as ref

EF = 6
GPU_MAIN = [(bits, metric) for bits in (1, 7) for metric in (0, 1)]  # the cases of tests/test_gpu_mstg_rerank.py
GPU_POOLS = (10, 40, 100, 4096)                                      # (100: top_k 100 at refine_pool 40)


# ---- anchor: every list selected, a pool that holds every (vector, list) pair --------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_anchor_whole_index_in_the_pool_is_the_argsort_of_the_canonical_distances(metric):
    import closure_cases as cc
    n, dim, k = 300, 32, 6
    x, c = cc.clustered(n, dim, k, 1234)
    case = rref.Case(x, c, 7, metric, 2.0, 8)
    assert len(case.pair_vec) <= 4096 and set(np.asarray(case.pair_vec).tolist()) == set(range(n))
    rng = np.random.default_rng(11)
    q = (x[rng.integers(0, n, 16)] + 0.05 * rng.standard_normal((16, dim))).astype(np.float32)
    lists, counts = rq.select_lists_cpu(q, case.c, k, 1e9)
    assert (counts == k).all()
    cands = rref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    assert all(np.isfinite(e).all() and len(e) == len(case.pair_vec) for _, e, _ in cands)
    ids, sc, cnt, ties = ref.rerank_ref(case.built, case.pair_vec, q, lists, counts, x, metric, n, 4096, cands)
    assert not any(ties) and (cnt == n).all()
    for i in range(len(q)):
        d = ref.distances(q[i], x, np.arange(n), metric)          # every row, not through the pool
        want = np.argsort(d, kind="stable")                        # (equal distances: the smaller id; checked distinct below)
        assert len(np.unique(d)) == n
        assert np.array_equal(ids[i], want.astype(np.uint64)), i
        assert np.array_equal(sc[i].view(np.uint32), d[want].view(np.uint32)), i
    # top_k below the number of ids: the head of the same order
    ids10, sc10, cnt10, _ = ref.rerank_ref(case.built, case.pair_vec, q, lists, counts, x, metric, 10, 4096, cands)
    assert (cnt10 == 10).all() and np.array_equal(ids10, ids[:, :10]) and np.array_equal(sc10.view(np.uint32), sc[:, :10].view(np.uint32))


# ---- the data of the GPU test ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,metric", GPU_MAIN, ids=lambda p: str(p))
def test_main_case_has_no_tie_at_a_cut_and_ids_twice_in_the_pool(bits, metric):
    case, q = rref.main_case(bits, metric)
    lists, counts = rq.select_lists_cpu(q, case.c, EF, 0.6)
    cands = rref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    for pool in GPU_POOLS:
        ids, sc, cnt, ties = ref.rerank_ref(case.built, case.pair_vec, q, lists, counts, case.x, metric, 10, pool, cands)
        assert not any(ties), pool
        for i in range(len(q)):
            c = int(cnt[i])
            assert len(set(ids[i, :c].tolist())) == c and (np.diff(sc[i, :c]) >= 0).all()
            assert (ids[i, c:] == ref.NONE64).all() and np.isnan(sc[i, c:]).all()
    # step 2 has work to do on this data: some pool holds an id more than once, and then fewer rows are read than entries pooled
    dup = 0
    for i, (cid, est, _) in enumerate(cands):
        *_, pool_ids, _tie, n_rows = ref.rerank_query(cid, est, q[i], case.x, metric, 10, 4096)
        assert n_rows == len(np.unique(pool_ids))
        dup += n_rows < len(pool_ids)
    assert dup > 0


def test_recall_exact_is_not_below_refined():
    """recall@10 at pool 100 against the truth by the same canonical distances.  A theorem, not a measurement: the exact top 10 of a
    pool holds every true neighbour the pool holds, and the refined hits are a subset of those."""
    case, q = rref.recall_case()
    lists, counts = rq.select_lists_cpu(q, case.c, 16, 0.6)
    n = len(case.x)
    truth = np.stack([np.argsort(ref.distances(q[i], case.x, np.arange(n), 0), kind="stable")[:10] for i in range(len(q))]).astype(np.uint64)
    cands = rref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    rid, _, rcnt, _, _ = rref.refine_ref(case.built, case.pair_vec, q, lists, counts, 0, 10, 100, cands)
    xid, _, xcnt, ties = ref.rerank_ref(case.built, case.pair_vec, q, lists, counts, case.x, 0, 10, 100, cands)
    assert not any(ties)
    refined, exact = rref.recall_at(rid, rcnt, truth), rref.recall_at(xid, xcnt, truth)
    print(f"recall@10 on the CPU restatement, pool 100: refined {refined:.4f} exact {exact:.4f}")
    assert exact >= refined


# ---- the refusal ---------------------------------------------------------------------------------------------------------------
def test_refusal_for_all_eight_combinations(tmp_path):
    exe = str(tmp_path / "mstg_rerank_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "mstg_rerank_check_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == 8
    seen = set()
    for row in rows:
        option, have_raw, rerank_on, rc, *detail = row.split(" ")
        option, have_raw, rerank_on, rc, detail = int(option), int(have_raw), int(rerank_on), int(rc), " ".join(detail)
        seen.add((option, have_raw, rerank_on))
        if not option or (have_raw and rerank_on):
            assert rc == _abi.RBQ_OK and detail == "", row
        else:
            assert rc == _abi.RBQ_INVALID_CONFIG and "mstg_rerank 0" in detail, row
            assert ("raw vectors attached" in detail) == (not have_raw), row   # (without rows that is what is said first)
            assert ("rerank 1" in detail) == bool(have_raw), row
    assert len(seen) == 8


# ---- header text -----------------------------------------------------------------------------------------------------------------
def test_headers_name_the_option_and_declare_nothing_new():
    rbq_h = open(os.path.join(ROOT, "include", "rbq.h")).read()
    start = rbq_h.index('"rerank_pool" v')
    assert '"mstg_rerank" 0/1' in rbq_h[start:rbq_h.index("int rbq_debug_set_option(", start)]  # in the option list
    mstg_h = open(os.path.join(ROOT, "include", "rbq_mstg.h")).read()
    assert '"mstg_rerank"' in mstg_h
    code = re.sub(r"/\*.*?\*/", "", mstg_h, flags=re.S)                      # what the compiler sees
    assert "mstg_rerank" not in code
    protos = re.findall(r"\b(rbq_\w+)\s*\(", code)
    assert protos == ["rbq_mstg_closure_assign", "rbq_mstg_build_device", "rbq_mstg_cluster_device", "rbq_hclustered_count",
                      "rbq_hclustered_centroids", "rbq_hclustered_offsets", "rbq_hclustered_members", "rbq_hclustered_stats",
                      "rbq_hclustered_free", "rbq_mstg_debug_closure_fallbacks", "rbq_mstg_debug_closure_shortlist", "rbq_mstg_search_batch", "rbq_mstg_search_batch_device",
                      "rbq_mstg_search_refined_batch", "rbq_mstg_search_refined_batch_device", "rbq_mstg_debug_search_fallbacks"]
    assert re.findall(r"^#define\s+(\w+)", code, flags=re.M) == ["RBQ_MSTG_H", "RBQ_MSTG_MAX_REPLICAS", "RBQ_MSTG_SHORTLIST",
                                                                "RBQ_MSTG_HOST_BELOW_DEFAULT", "RBQ_MSTG_HOST_BELOW",
                                                                "RBQ_MSTG_SEARCH_SHORTLIST", "RBQ_MSTG_REFINE_POOL_MAX"]
