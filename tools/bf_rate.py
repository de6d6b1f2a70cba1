"""Rate of the brute-force index (rbq_bf_search_batch): N = 200 000, dim 1024, 7 bits, L2, FhtKac with the faster config, built
on the CPU builder; 1024-query calls from page-locked buffers, top_k = 10.  Warm-up, then the median of the repeats.  8 of the
queries are checked against the numpy restatement (tests/bf_ref.py).  Prints one JSON line.  Kernel time: run under
rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=8)
    a = ap.parse_args()
    import rabitq_rs_amd as rq
    from rabitq_rs_amd import bruteforce as bfm
    rng = np.random.default_rng(2024)
    data = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    t0 = time.time()
    built = rq.builder.train_bruteforce(data, 7, rq.Metric.L2, rq.RotatorType.FhtKacRotator, 7, True)
    t_build = time.time() - t0
    idx = rq.BruteForceRabitqIndex.from_built(built)
    L = bfm.lib()
    k, nq, dim = a.top_k, a.nq, a.dim
    nbytes = nq * dim * 4 + nq * k * 12 + nq * 4
    base = L.rbq_host_alloc(nbytes)
    assert base
    q = np.ctypeslib.as_array(C.cast(base, C.POINTER(C.c_float)), shape=(nq, dim))
    q[:] = rng.standard_normal((nq, dim)).astype(np.float32)
    p_ids = base + nq * dim * 4
    p_sc = p_ids + nq * k * 8
    p_cnt = p_sc + nq * k * 4
    times = []
    for i in range(a.warmup + a.repeats):
        t = time.perf_counter()
        rc = L.rbq_bf_search_batch(idx._h, q.ctypes.data, nq, dim, k, None, 0, p_ids, p_sc, p_cnt)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        if i >= a.warmup:
            times.append(dt)
    ids = np.ctypeslib.as_array(C.cast(p_ids, C.POINTER(C.c_uint64)), shape=(nq, k)).copy()
    sc = np.ctypeslib.as_array(C.cast(p_sc, C.POINTER(C.c_float)), shape=(nq, k)).copy()
    import bf_ref
    prep = bf_ref.Prepared(built.hdr_ptr, built.arrays())
    ok = 0
    for i in np.linspace(0, nq - 1, a.check).astype(int):
        rid, rsc = bf_ref.search(prep, q[i], k)
        ok += int(np.array_equal(ids[i, :len(rid)], rid) and np.array_equal(sc[i, :len(rid)].view(np.uint32), rsc.view(np.uint32)))
    L.rbq_host_free(base)
    ms = float(np.median(times)) * 1e3
    pairs = nq * a.n
    bound_ms = pairs * 3 * dim / 78.6e12 * 1e3
    print(json.dumps({"tool": "bf_rate", "n": a.n, "dim": dim, "bits": 7, "nq_per_call": nq, "top_k": k, "repeats": a.repeats,
                      "ms_per_call": round(ms, 3), "queries_per_s": round(nq / ms * 1e3, 1),
                      "valu_bound_ms": round(bound_ms, 3), "fraction_of_bound": round(bound_ms / ms, 4),
                      "checked": int(a.check), "checked_equal": ok, "build_s": round(t_build, 1)}))
    return 0 if ok == a.check else 1


if __name__ == "__main__":
    sys.exit(main())
