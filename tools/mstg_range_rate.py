"""Time of the MSTG range search (rbq_mstg_range_batch*) next to the top-k search (rbq_mstg_search_batch*) on one handle: N = 1 M
vectors of dim 960, 7 bits, L2, batches of 1024 device-resident queries, the `balanced` preset (ef_search 150, pruning_epsilon
0.6), about 1000 lists.  The radius is the median over the batch of the --kth smallest estimate (--kth 100 is the shape to record),
so a query has about that many matches; the top-k leg runs at top_k = the median match count, which is what a caller without a
range search would have to guess.  One process per shape, under a time limit of its own, nothing started after a failure:

  timeout -k 10 900 python tools/mstg_range_rate.py --kth 100 --out profiles/mstg_range/rate_kth100.json
  timeout -k 10 1100 python tools/mstg_range_rate.py --kth 100 --exact --out profiles/mstg_range_exact/rate_kth100.json
  timeout -k 10 1100 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mstg_range_rate.py --kth 100 --exact \
      --windows 1 --calls 3 --out DIR/rate.json && python tools/mstg_range_rate.py --kernel-table DIR --out profiles/mstg_range_exact/kernels_kth100.json

Every leg is a device-entry call timed between stream synchronisations: one warm-up window, then the median of --windows windows
of --calls calls each.  The same legs on the parent commit's library give the comparison for `mstg_search` (the range legs do not
exist there).  Recorded: profiles/mstg_range_exact/rate_kth100.json (the run with --exact, which holds the estimate-only legs too)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def windows(fn, sync, n_windows, calls):
    """seconds per call: the median over n_windows windows of `calls` calls, after one warm-up window"""
    out = []
    for w in range(n_windows + 1):
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / calls)
    return {"median_s": statistics.median(out[1:]), "min_s": min(out[1:]), "max_s": max(out[1:])}


def exact_legs(rq, idx, x, q, tq, sel, a, sync):
    """--exact: the exact range search (mstg_range_rows(..., exact=True)) on the same index and batch.  The
    exact radius is the median over the batch of the --kth smallest exact distance (the exact rerank of a pool of 4096), the
    candidate radius r is that value and 1.05 times it, the rows are attached as f32 and as f16; every exact leg stands next to
    the estimate-only distinct call at the same r, timed in the same run."""
    out = []
    for raw in ("f32", "f16"):
        idx.set_rerank_vectors(x, dtype=raw)
        _, d, cnt = rq.mstg_search(idx, q, a.kth, *sel, refine_pool=4096, exact=True)
        xr = float(np.median(d[cnt >= a.kth, a.kth - 1]))
        for r in (xr, 1.05 * xr):
            cand = rq.mstg_range_rows(idx, q, r, 1, *sel, distinct=True)[2].astype(np.int64)
            hit = rq.mstg_range_rows(idx, q, xr, 1, *sel, exact=True, candidate_radius=r)[2].astype(np.int64)
            ok = cand != 0xFFFFFFFF
            cap = max(int(cand[ok].max()) if ok.any() else 1, 1)
            leg = {"raw": raw, "exact_radius": xr, "candidate_radius": r, "over_distinct_limit": int((~ok).sum()), "capacity": cap,
                   "candidates_median": int(np.median(cand[ok])) if ok.any() else 0, "matches_median": int(np.median(hit[ok])) if ok.any() else 0}
            leg["range_distinct"] = windows(lambda: rq.mstg_range_rows(idx, tq, r, cap, *sel, distinct=True), sync, a.windows, a.calls)
            leg["range_exact"] = windows(lambda: rq.mstg_range_rows(idx, tq, xr, cap, *sel, exact=True, candidate_radius=r), sync, a.windows, a.calls)
            out.append(leg)
    idx.set_rerank_vectors(None)
    return out


def kernel_table(a):
    """--kernel-table DIR: the range kernels' times from the *kernel_trace.csv files a `rocprofv3 --kernel-trace --stats -d DIR --`
    run of this tool (its own run, few windows) left under DIR: per kernel the dispatches and their median / min / max in
    microseconds.  The legs of a run share kernels, so a kernel's dispatches mix the radii of its legs."""
    import csv
    import glob
    us = {}
    for f in glob.glob(os.path.join(a.kernel_table, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_mstg_range" in r["Kernel_Name"]:
                name = r["Kernel_Name"].split("(")[0].replace("void rbq::", "")
                us.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rec = {"source": "rocprofv3 --kernel-trace, a run of its own",
           "kernels": {k: {"dispatches": len(v), "median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                       for k, v in sorted(us.items())}}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kth", type=int, default=100)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--exact", action="store_true", help="add the exact legs (see exact_legs)")
    ap.add_argument("--kernel-table", default=None, metavar="DIR", help="no run: tabulate the kernel trace under DIR (see kernel_table)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.kernel_table:
        return kernel_table(a)
    import torch
    import rabitq_rs_amd as rq
    from mstg_build_rate import dataset
    p = rq.MstgSearchParams.balanced()
    k = a.lists * a.n // 1000000 or 1
    x = dataset(a.n, a.dim, 32, 1)
    cent = np.ascontiguousarray(x[:: a.n // k][:k])
    rng = np.random.default_rng(2)
    q = (x[rng.integers(0, a.n, a.batch)] + 0.02 * rng.standard_normal((a.batch, a.dim))).astype(np.float32)
    idx = rq.build_postings_on_device(x, cent, 7, 0, faster_config=True)
    sel = (p.ef_search, p.pruning_epsilon)
    _, est, cnt = rq.mstg_search(idx, q, a.kth, *sel)
    radius = float(np.median(est[cnt >= a.kth, a.kth - 1]))
    rec = {"n": a.n, "dim": a.dim, "n_lists": k, "batch": a.batch, "ef_search": sel[0], "pruning_epsilon": sel[1], "kth": a.kth,
           "radius": radius, "windows": a.windows, "calls": a.calls, "stored_vectors": len(idx)}
    raw = rq.mstg_range_rows(idx, q, radius, 1, *sel, distinct=False)[2].astype(np.int64)
    uniq = rq.mstg_range_rows(idx, q, radius, 1, *sel, distinct=True)[2].astype(np.int64)
    rec["matches_median"], rec["matches_max"] = int(np.median(raw)), int(raw.max())
    rec["over_distinct_limit"] = int((uniq == 0xFFFFFFFF).sum())
    rec["distinct_median"] = int(np.median(uniq[uniq != 0xFFFFFFFF])) if (uniq != 0xFFFFFFFF).any() else 0
    cap = max(int(raw.max()), 1)
    top_k = max(rec["matches_median"], 1)
    tq = torch.from_numpy(q).cuda()
    sync = torch.cuda.synchronize
    rec["capacity"], rec["top_k"] = cap, top_k
    rec["range_raw"] = windows(lambda: rq.mstg_range_rows(idx, tq, radius, cap, *sel, distinct=False), sync, a.windows, a.calls)
    rec["range_distinct"] = windows(lambda: rq.mstg_range_rows(idx, tq, radius, cap, *sel, distinct=True), sync, a.windows, a.calls)
    rec["search_top_k"] = windows(lambda: rq.mstg_search(idx, tq, top_k, *sel), sync, a.windows, a.calls)
    if a.exact:
        rec["exact"] = exact_legs(rq, idx, x, q, tq, sel, a, sync)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
