"""Time of the exact rerank of the MSTG pool (option "mstg_rerank") next to the refined and the plain MSTG
search on one handle: N = 1 M vectors of dim 960, 7 bits, L2, batches of 1024 queries, the `balanced` preset (ef_search 150,
pruning_epsilon 0.6), about 1000 lists.  One (pool, row type) per process, each step under a time limit of its own, and nothing is
started after a failure; the kernel's own time comes from a kernel-trace run of its own:

  timeout -k 10 900 python tools/mstg_rerank_rate.py --pool 100 --raw-dtype f32 --out profiles/mstg_rerank/rate_pool100_f32.json &&
  timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mstg_rerank_rate.py --pool 100 \
      --raw-dtype f32 --traced --out DIR/traced.json &&
  python tools/mstg_rerank_rate.py --kernel-table DIR --rate profiles/mstg_rerank/rate_pool100_f32.json \
      --out profiles/mstg_rerank/kernel_pool100_f32.json

and the same for --pool 1000 and --raw-dtype f16.  Every leg of the rate run is the wall time of the whole call, one warm-up run
and then the median of --repeats runs, on the host entry and on the device entry (timed between stream synchronisations).  The
record also holds the mean number of distinct ids per pool: the kernel's requested bytes are distinct ids x dim x element size."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ELEM_BYTES = {"f32": 4, "f16": 2}


def kernel_table(a):
    rate = json.load(open(a.rate))
    traced = json.load(open(os.path.join(a.kernel_table, "traced.json")))
    rows = []
    for f in glob.glob(os.path.join(a.kernel_table, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "k_mstg_rerank" in r["Kernel_Name"]]
    if len(rows) != traced["calls"]:
        raise SystemExit(f"unexpected dispatch count: k_mstg_rerank {len(rows)}, calls {traced['calls']}")
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    med = statistics.median(us)
    req = rate["distinct_ids_per_batch"] * rate["dim"] * ELEM_BYTES[rate["raw_dtype"]]
    rec = {"source": "rocprofv3 --kernel-trace, a run of its own", "kernel": rows[0]["Kernel_Name"], "refine_pool": rate["refine_pool"],
           "raw_dtype": rate["raw_dtype"], "dispatches": len(us), "median_us": round(med, 2), "min_us": round(min(us), 2),
           "max_us": round(max(us), 2), "requested_bytes": req, "requested_TBps": round(req / (med * 1e-6) / 1e12, 3)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--raw-dtype", choices=tuple(ELEM_BYTES), default="f32")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--traced", action="store_true", help="only the exact device calls (--repeats of them, after one warm-up)")
    ap.add_argument("--kernel-table", default=None, metavar="DIR")
    ap.add_argument("--rate", default=None)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.kernel_table:
        return kernel_table(a)
    import torch
    import rabitq_rs_amd as rq
    from mstg_build_rate import dataset
    from mstg_search_rate import timed
    p = rq.MstgSearchParams.balanced()
    k = a.lists * a.n // 1000000 or 1
    x = dataset(a.n, a.dim, 32, 1)
    cent = np.ascontiguousarray(x[:: a.n // k][:k])
    rng = np.random.default_rng(2)
    q = (x[rng.integers(0, a.n, a.batch)] + 0.02 * rng.standard_normal((a.batch, a.dim))).astype(np.float32)
    idx = rq.build_postings_on_device(x, cent, 7, 0, faster_config=True)
    idx.set_rerank_vectors(x.astype(np.float16) if a.raw_dtype == "f16" else x, dtype=a.raw_dtype)
    args = (a.top_k, p.ef_search, p.pruning_epsilon)
    tq = torch.from_numpy(q).cuda()

    def dev(**kw):
        rq.mstg_search(idx, tq, *args, **kw)
        torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.traced:
        dev(refine_pool=a.pool, exact=True)  # (warm-up: the one-time maps and the LDS attribute)
        for _ in range(a.repeats):
            dev(refine_pool=a.pool, exact=True)
        rec = {"calls": a.repeats + 1, "refine_pool": a.pool, "raw_dtype": a.raw_dtype}
    else:
        rec = {"n": a.n, "dim": a.dim, "n_lists": k, "batch": a.batch, "top_k": a.top_k, "ef_search": p.ef_search,
               "pruning_epsilon": p.pruning_epsilon, "refine_pool": a.pool, "raw_dtype": a.raw_dtype, "stored_vectors": len(idx)}
        pool = max(a.pool, a.top_k)
        pids, _, pcnt = rq.mstg_search(idx, q, pool, p.ef_search, p.pruning_epsilon)  # the pool itself: the plain call at top_k := pool
        rec["distinct_ids_per_batch"] = int(sum(len(set(pids[i, :int(pcnt[i])].tolist())) for i in range(len(q))))
        rec["pool_entries_per_batch"] = int(pcnt.sum())
        xi, _, xc = rq.mstg_search(idx, q, *args, refine_pool=a.pool, exact=True)
        rec["exact_rows_unique"] = bool(all(len(set(xi[i, :int(xc[i])].tolist())) == int(xc[i]) for i in range(len(q))))
        rec["exact_mean_count"] = round(float(xc.mean()), 3)
        rec["plain_host"] = timed(lambda: rq.mstg_search(idx, q, *args), a.repeats)
        rec["refined_host"] = timed(lambda: rq.mstg_search(idx, q, *args, refine_pool=a.pool), a.repeats)
        rec["exact_host"] = timed(lambda: rq.mstg_search(idx, q, *args, refine_pool=a.pool, exact=True), a.repeats)
        rec["plain_device"] = timed(lambda: dev(), a.repeats)
        rec["refined_device"] = timed(lambda: dev(refine_pool=a.pool), a.repeats)
        rec["exact_device"] = timed(lambda: dev(refine_pool=a.pool, exact=True), a.repeats)
    idx.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
