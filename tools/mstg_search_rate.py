"""Search time of an MSTG handle in one call (rbq_mstg_search_batch, rbq_mstg_search_batch_device) against the two-step path
it replaces: select_lists_cpu on OMP_NUM_THREADS threads followed by rbq_posting_scan_batch.  N = 1 M vectors of dim 960,
7 bits, L2, batches of 1024 queries, the `balanced` preset (ef_search 150, pruning_epsilon 0.6).  Two shapes (--shape):

  lists1k    about 1000 lists (the Rust default's regime)
  lists60k   about 60 000 lists (the Python default max_posting_size = 16)

Centroids are every (N / n_lists)-th row of the data and the handle is built by build_postings_on_device, so that no leg
needs a clustering step.  One process per shape, so that every GPU step runs under a time limit of its own and nothing is
started after a failure (tools/mstg_search_rate.sh):

  timeout -k 10 900 python tools/mstg_search_rate.py --shape lists1k  --out profiles/mstg_search_rate_lists1k.json &&
  timeout -k 10 900 python tools/mstg_search_rate.py --shape lists60k --out profiles/mstg_search_rate_lists60k.json

Every leg is the wall time of the whole call, one warm-up run and then the median of --repeats runs; the device leg is
timed between stream synchronisations.  The record holds the stage times, the mean number of selected lists per query and
the fallback queries; the host call is checked against the two-step path before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"lists1k": 1000, "lists60k": 62500}


def timed(fn, repeats, warmup=1):
    times = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * float(np.median(times)), 3), "min_ms": round(1e3 * min(times), 3), "max_ms": round(1e3 * max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    from rabitq_rs_amd import mstg
    from mstg_build_rate import dataset
    p = rq.MstgSearchParams.balanced()
    k = SHAPES[a.shape] * a.n // 1000000 or 1
    x = dataset(a.n, a.dim, 32, 1)
    cent = np.ascontiguousarray(x[:: a.n // k][:k])
    rng = np.random.default_rng(2)
    q = (x[rng.integers(0, a.n, a.batch)] + 0.02 * rng.standard_normal((a.batch, a.dim))).astype(np.float32)
    t0 = time.perf_counter()
    idx = rq.build_postings_on_device(x, cent, 7, 0, faster_config=True)
    rec = {"shape": a.shape, "n": a.n, "dim": a.dim, "n_lists": k, "batch": a.batch, "top_k": a.top_k, "ef_search": p.ef_search,
           "pruning_epsilon": p.pruning_epsilon, "threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "stored_vectors": len(idx),
           "build_s": round(time.perf_counter() - t0, 2)}
    fb0 = mstg.search_fallbacks()
    ids, sc, cnt, li, lc = rq.mstg_search(idx, q, a.top_k, p.ef_search, p.pruning_epsilon, return_lists=True)
    rec["fallback_queries"] = mstg.search_fallbacks() - fb0
    rec["mean_selected_lists"] = round(float(lc.mean()), 2)
    rl, rc = rq.select_lists_cpu(q, cent, p.ef_search, p.pruning_epsilon)
    pids, psc, pcnt = idx.posting_scan(q, a.top_k, rl, rc)
    rec["equal_to_two_step"] = bool(np.array_equal(li, rl) and np.array_equal(lc, rc) and np.array_equal(ids, pids) and
                                    np.array_equal(sc.view(np.uint32), psc.view(np.uint32)) and np.array_equal(cnt, pcnt))
    rec["one_call_host"] = timed(lambda: rq.mstg_search(idx, q, a.top_k, p.ef_search, p.pruning_epsilon), a.repeats)
    tq = torch.from_numpy(q).cuda()

    def dev():
        rq.mstg_search(idx, tq, a.top_k, p.ef_search, p.pruning_epsilon)
        torch.cuda.synchronize()
    rec["one_call_device"] = timed(dev, a.repeats)
    rec["two_step_select_cpu"] = timed(lambda: rq.select_lists_cpu(q, cent, p.ef_search, p.pruning_epsilon), a.repeats)
    rec["two_step_posting_scan"] = timed(lambda: idx.posting_scan(q, a.top_k, rl, rc), a.repeats)
    rec["two_step_total_median_ms"] = round(rec["two_step_select_cpu"]["median_ms"] + rec["two_step_posting_scan"]["median_ms"], 3)
    idx.profile_begin()
    rq.mstg_search(idx, q, a.top_k, p.ef_search, p.pruning_epsilon)
    idx.profile_end()
    rec["stage_ms"] = {name: round(idx.profile_stage(stage)[0], 3) for name, stage in
                       (("prep", "prep"), ("select", "rank"), ("work_list", "select"), ("scan", "scan"))}
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
