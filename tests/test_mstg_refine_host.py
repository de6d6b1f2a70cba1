"""The refined MSTG search without a GPU: the NumPy restatement tests/mstg_refine_ref.py is anchored to the oracle twice (its
binary stage to oracle.posting_scan_batch, its refined distances to oracle.search_batch), the data of the GPU tests is shown to
exercise what they are about (an id twice in a binary pool; refined recall not below the plain one), and the C ABI's new
symbols and argument errors are checked on the host (the errors need no device: rbq_host::mstg_search_check)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
from conftest import ROOT
from rabitq_rs_amd import _abi, index as ix
import mstg_refine_ref as ref

HOST = os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host")
MAIN = [(bits, metric) for bits in (1, 3, 7) for metric in (0, 1)]
EF = 6


@pytest.fixture(scope="module", params=MAIN, ids=lambda p: "bits%d_metric%d" % p)
def main(request):
    bits, metric = request.param
    case, q = ref.main_case(bits, metric)
    sel = {eps: rq.select_lists_cpu(q, case.c, EF, eps) for eps in (0.6, 1e9)}
    return case, q, sel


def test_binary_stage_is_the_oracles_posting_scan(main):
    case, q, sel = main
    mask = np.uint32(0x7fffffff if case.metric == 0 else 0xffffffff)
    for eps, (lists, counts) in sel.items():
        for pool in (10, 40, 4096):
            rc, _, osc, ocnt = oracle.posting_scan_batch(case.built, q, pool, lists, counts)
            assert rc == 0
            _, _, _, pools, _ = ref.refine_ref(case.built, case.pair_vec, q, lists, counts, case.metric, 1, pool)
            for i in range(len(q)):
                e = pools[i][1]
                assert len(e) == ocnt[i], (eps, pool, i)
                assert np.array_equal(e.view(np.uint32) & mask, osc[i, :len(e)].view(np.uint32) & mask), (eps, pool, i)


def test_refined_distances_are_the_oracles_search_scores(main):
    """oracle.search_batch over the same lists with every list probed and a heap that never fills: nothing is pruned, and every
    vector's score is its refined distance (negated for inner product)."""
    case, q, _ = main
    built = case.built
    k, total = built.n_lists, len(built)
    qs = q[:6]
    rc, oids, osc, ocnt, _ = oracle.search_batch(built, qs, total + 1, k)
    assert rc == 0
    all_lists = np.arange(k, dtype=np.uint32)
    for i in range(len(qs)):
        pid, _, dist = ref.candidates(built, np.arange(total), qs[i], all_lists, k)  # (ids: the pair indices themselves)
        fin = np.isfinite(dist)
        assert ocnt[i] == fin.sum() == total
        by_pair = np.empty(total, np.float32)
        by_pair[oids[i, :total].astype(np.int64)] = osc[i, :total] if case.metric == 0 else -osc[i, :total]
        assert np.array_equal(by_pair[pid.astype(np.int64)].view(np.uint32), dist.view(np.uint32)), i


def test_main_case_has_an_id_twice_in_a_binary_pool(main):
    """... for every pool size of the GPU test, and no estimate tie sits at a pool's cut (the scan's heap would decide it)"""
    case, q, sel = main
    for eps, (lists, counts) in sel.items():
        for pool in (10, 40, 4096):
            _, _, _, pools, ties = ref.refine_ref(case.built, case.pair_vec, q, lists, counts, case.metric, 10, pool)
            assert not any(ties), (eps, pool)
            dup = [i for i, (pid, _) in enumerate(pools) if len(np.unique(pid)) < len(pid)]
            assert dup, (eps, pool)


def test_rows_are_unique_sorted_and_padded(main):
    case, q, sel = main
    lists, counts = sel[0.6]
    ids, sc, cnt, _, _ = ref.refine_ref(case.built, case.pair_vec, q, lists, counts, case.metric, 10, 40)
    for i in range(len(q)):
        c = int(cnt[i])
        assert len(set(ids[i, :c].tolist())) == c and (np.diff(sc[i, :c]) >= 0).all()
        assert (ids[i, c:] == ref.NONE64).all() and np.isnan(sc[i, c:]).all()


def test_recall_case_refined_is_not_below_plain():
    case, q = ref.recall_case()
    lists, counts = rq.select_lists_cpu(q, case.c, 16, 0.6)
    d2 = ((q[:, None, :].astype(np.float64) - case.x[None, :, :].astype(np.float64)) ** 2).sum(-1)
    truth = np.argsort(d2, axis=1, kind="stable")[:, :10].astype(np.uint64)
    # the plain call: the 10 best binary entries, an id possibly several times
    _, _, _, pools, _ = ref.refine_ref(case.built, case.pair_vec, q, lists, counts, 0, 10, 0)
    plain_ids = np.full((len(q), 10), ref.NONE64, np.uint64)
    plain_cnt = np.zeros(len(q), np.uint32)
    for i, (pid, _) in enumerate(pools):
        plain_ids[i, :len(pid)] = pid
        plain_cnt[i] = len(pid)
    ids, _, cnt, _, _ = ref.refine_ref(case.built, case.pair_vec, q, lists, counts, 0, 10, 100)
    plain, refined = ref.recall_at(plain_ids, plain_cnt, truth), ref.recall_at(ids, cnt, truth)
    print(f"recall@10 on the CPU restatement: plain {plain:.4f} refined (pool 100) {refined:.4f}")
    assert refined >= plain


# ---- the C ABI on the host ------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    L = ix.lib()
    for name in ("rbq_mstg_search_refined_batch", "rbq_mstg_search_refined_batch_device"):
        assert getattr(L, name).restype is C.c_int
    hdr = open(os.path.join(ROOT, "include", "rbq_mstg.h")).read()
    assert "int rbq_mstg_search_refined_batch(" in hdr and "int rbq_mstg_search_refined_batch_device(" in hdr
    assert "#define RBQ_MSTG_REFINE_POOL_MAX 4096" in hdr
    assert L.rbq_abi_version() == (2 << 16) | 2


def test_null_index_is_refused_before_any_device_call():
    L = ix.lib()
    q = np.zeros((1, 16), np.float32)
    ids, sc, cnt = np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.float32), np.zeros(1, np.uint32)
    rc = L.rbq_mstg_search_refined_batch(None, q.ctypes.data, 1, 16, 4, 6, 0.6, 40, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None)
    assert rc == _abi.RBQ_INVALID_CONFIG and ix._detail() == "null index"
    rc = L.rbq_mstg_search_refined_batch_device(None, q.ctypes.data, 1, 16, 4, 6, 0.6, 40, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data,
                                                None, None, None)
    assert rc == _abi.RBQ_INVALID_CONFIG and ix._detail() == "null index"


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "librbq_hostcheck.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), "-shared", "-o", out,
                           os.path.join(HOST, "rbq_hostcheck.cpp")])
    L = C.CDLL(out)
    L.rbq_hostcheck_mstg_search_args.restype = C.c_int
    L.rbq_hostcheck_mstg_search_args.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32,
                                                 C.c_char_p, C.c_size_t, C.c_void_p]
    return L


HANDLE, QUERIES, IDS, SCORES, COUNTS, REFINED = 1, 2, 4, 8, 16, 32
ALL = HANDLE | QUERIES | IDS | SCORES | COUNTS


def _check(L, flags=ALL | REFINED, n_vectors=100, dim=16, query_dim=16, rotator=2, nq=3, top_k=10, refine_pool=40):
    det = C.create_string_buffer(256)
    out = (C.c_uint32 * 2)()
    rc = L.rbq_hostcheck_mstg_search_args(flags, n_vectors, dim, query_dim, rotator, nq, top_k, refine_pool, det, 256, out)
    return rc, det.value.decode(), int(out[0]), int(out[1])


def test_argument_errors_come_in_the_stated_order(hostcheck):
    """every later error is present in each call: the earliest one is reported"""
    L = hostcheck
    bad = dict(n_vectors=0, query_dim=17, rotator=1, nq=3, top_k=(1 << 20) + 1, refine_pool=5000)
    assert _check(L, flags=REFINED, **bad)[:2] == (_abi.RBQ_INVALID_CONFIG, "null index")
    assert _check(L, flags=HANDLE | REFINED, **bad)[:2] == (_abi.RBQ_EMPTY_INDEX, "index is empty")
    bad["n_vectors"] = 100
    assert _check(L, flags=HANDLE | REFINED, **bad)[:2] == (_abi.RBQ_DIMENSION_MISMATCH, "expected 16, got 17")
    bad["query_dim"] = 16
    assert _check(L, flags=HANDLE | REFINED, **bad)[:2] == (_abi.RBQ_INVALID_CONFIG, "MSTG search needs an index created with rotator NONE")
    bad["rotator"] = 2
    assert _check(L, flags=HANDLE | REFINED, **dict(bad, nq=0)) == (_abi.RBQ_OK, "", 1, 0)  # nq == 0 answers the call
    for missing in (QUERIES, COUNTS, IDS, SCORES):
        assert _check(L, flags=(ALL & ~missing) | REFINED, **bad)[:2] == (_abi.RBQ_INVALID_CONFIG, "null buffer")
    assert _check(L, flags=HANDLE | QUERIES | COUNTS | REFINED, **dict(bad, top_k=0))[0] == _abi.RBQ_INVALID_CONFIG  # (pool 5000)
    assert _check(L, flags=HANDLE | QUERIES | COUNTS | REFINED, top_k=0, refine_pool=40) == (_abi.RBQ_OK, "", 0, 40)
    assert _check(L, **bad)[:2] == (_abi.RBQ_INVALID_CONFIG, "top_k too large for one call (top_k <= 2^20)")
    bad["top_k"] = 10
    rc, msg, _, _ = _check(L, **bad)
    assert rc == _abi.RBQ_INVALID_CONFIG and msg == "refine pool too large: max(refine_pool, top_k) <= 4096"


def test_pool_is_the_larger_of_refine_pool_and_top_k(hostcheck):
    L = hostcheck
    assert _check(L, top_k=10, refine_pool=0) == (_abi.RBQ_OK, "", 0, 10)
    assert _check(L, top_k=10, refine_pool=4096) == (_abi.RBQ_OK, "", 0, 4096)
    assert _check(L, top_k=4096, refine_pool=0) == (_abi.RBQ_OK, "", 0, 4096)
    assert _check(L, top_k=10, refine_pool=4097)[0] == _abi.RBQ_INVALID_CONFIG
    assert _check(L, top_k=4097, refine_pool=0)[0] == _abi.RBQ_INVALID_CONFIG
    # the plain call has no pool: the same arguments pass
    assert _check(L, flags=ALL, top_k=4097, refine_pool=0) == (_abi.RBQ_OK, "", 0, 0)
    assert _check(L, flags=ALL, top_k=10, refine_pool=10 ** 6) == (_abi.RBQ_OK, "", 0, 0)
