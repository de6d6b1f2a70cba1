"""Time of the brute-force range search (rbq_bf_range_batch) next to the top-k search (rbq_bf_search_batch) on one handle: the
index of tools/bf_mutate_rate.py (200 000 x 1024 Gaussian rows, 7 bits, L2, trained on the device), batches of 1024 host queries,
the radius at the median over the batch of the --kth (100) smallest distance, so a query has about that many matches.  One
process, under a time limit of its own, nothing started after a failure:

  timeout -k 10 900 python tools/bf_range_rate.py --out profiles/bf_range/rate.json
  timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bf_range_rate.py --windows 1 --calls 1 \
      --out DIR/rate.json && python tools/bf_range_rate.py --kernel-table DIR --out profiles/bf_range/kernels.json

Every leg is a host-buffer call, which ends in a stream synchronisation: one warm-up window, then the median of --windows windows
of --calls calls each.  Legs: range_rows at capacity 1024, count_in_range, and batch_search_raw at top_k 100 and 1024 in the same
run as the comparison."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, n_windows, calls):
    """seconds per call: the median over n_windows windows of `calls` calls, after one warm-up window"""
    out = []
    for w in range(n_windows + 1):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls)
    return {"median_s": statistics.median(out[1:]), "min_s": min(out[1:]), "max_s": max(out[1:])}


def kernel_table(a):
    """--kernel-table DIR: the brute-force kernels' device times from the *kernel_trace.csv files a `rocprofv3 --kernel-trace --stats
    -d DIR --` run of this tool (its own run, one window) left under DIR: per kernel the dispatches, their median and their sum in
    microseconds.  k_bf_dist runs under every leg; the two range kernels under the range legs only."""
    import csv
    import glob
    us = {}
    for f in glob.glob(os.path.join(a.kernel_table, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_bf_" in r["Kernel_Name"]:
                name = r["Kernel_Name"].split("(")[0].replace("void rbq::", "")
                us.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rec = {"source": "rocprofv3 --kernel-trace, a run of its own",
           "kernels": {k: {"dispatches": len(v), "median_us": round(statistics.median(v), 1), "sum_us": round(sum(v), 1)} for k, v in sorted(us.items())}}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def exact_legs(a, idx, rows, q, rec):
    """--exact: rbq_bf_range_exact_batch over the training rows attached as f32 and as f16 (borrowed device
    tensors), x at the median over the batch of the --kth smallest exact distance, the candidate radius at x, 1.05 x and +inf (every
    vector scored: three windows of one call), each next to the estimate-only range_rows at the same radius in the same run."""
    import torch
    d2 = torch.cdist(torch.from_numpy(q).cuda(), rows).square_()
    x = float(d2.kthvalue(a.kth, dim=1).values.median())
    del d2
    rec["exact_x"] = x
    for name, r in (("r_1.00x", x), ("r_1.05x", 1.05 * x), ("r_inf", float("inf"))):
        n_win, calls = (a.windows, a.calls) if np.isfinite(r) else (min(a.windows, 3), 1)
        rec["estimate_" + name] = dict(windows(lambda: idx.range_rows(q, r, a.capacity), n_win, calls),
                                       candidates_median=int(np.median(idx.count_in_range(q, r))))
        for raw, stored in (("f32", rows), ("f16", rows.half())):
            idx.set_rerank_vectors(stored)
            leg = windows(lambda: idx.range_rows(q, r, a.capacity, exact_x=x), n_win, calls)
            leg["matches_median"] = int(np.median(idx.range_rows(q, r, 0, exact_x=x)[2]))
            rec["exact_%s_%s" % (raw, name)] = leg
            idx.set_rerank_vectors(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--kth", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--exact", action="store_true", help="the legs of the exact range search instead (see exact_legs)")
    ap.add_argument("--kernel-table", default=None, metavar="DIR", help="no run: tabulate the kernel trace under DIR (see kernel_table)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.kernel_table:
        return kernel_table(a)
    import torch
    import rabitq_rs_amd as rq
    if not torch.cuda.is_available():
        sys.exit("bf_range_rate needs a GPU: nothing is measured without one")
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    x = torch.randn((a.n, a.dim), generator=g, device="cuda", dtype=torch.float32)
    idx = rq.BruteForceRabitqIndex.train_on_device(x, a.bits, 0, 1, a.seed, True)  # (L2, FHT-Kac rotator, faster config)
    rng = np.random.default_rng(a.seed)
    q = (x[torch.from_numpy(rng.integers(0, a.n, a.batch)).cuda()].cpu().numpy() + 0.5 * rng.standard_normal((a.batch, a.dim))).astype(np.float32)
    if not a.exact:
        del x
    _, d, cnt = idx.batch_search_raw(q, rq.BruteForceSearchParams(a.kth))
    radius = float(np.median(d[cnt >= a.kth, a.kth - 1]))
    totals = idx.count_in_range(q, radius).astype(np.int64)
    rec = {"tool": "bf_range_rate", "n": a.n, "dim": a.dim, "bits": a.bits, "metric": "l2", "batch": a.batch, "kth": a.kth, "radius": radius,
           "capacity": a.capacity, "windows": a.windows, "calls": a.calls, "matches_median": int(np.median(totals)),
           "matches_max": int(totals.max()), "rows_cut": int((totals > a.capacity).sum())}
    if a.exact:
        exact_legs(a, idx, x, q, rec)
    else:
        rec["range_rows"] = windows(lambda: idx.range_rows(q, radius, a.capacity), a.windows, a.calls)
        rec["count_in_range"] = windows(lambda: idx.count_in_range(q, radius), a.windows, a.calls)
        for k in (100, 1024):
            rec["search_top_k_%d" % k] = windows(lambda: idx.batch_search_raw(q, rq.BruteForceSearchParams(k)), a.windows, a.calls)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
