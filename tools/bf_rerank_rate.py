"""Time and recall of the exact brute-force top-k (rbq_bf_search_exact_batch) next to the estimate-only search
(rbq_bf_search_batch) on one handle: the index of tools/bf_range_rate.py (200 000 x 1024 Gaussian rows, 7 bits, L2, trained on the
device), batches of 1024 page-locked host queries.  One process, under a time limit of its own, nothing started after a failure:

  timeout -k 10 900 python tools/bf_rerank_rate.py --out profiles/bf_rerank/rate.json
  timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bf_rerank_rate.py --windows 1 --calls 1 \
      --pools 1024 --out DIR/rate.json && python tools/bf_rerank_rate.py --kernel-table DIR --out profiles/bf_rerank/kernels.json

Every leg is a host-buffer call, which ends in a stream synchronisation: one warm-up window, then the median of --windows windows
of --calls calls each.  Legs, per pool of --pools: batch_search_raw at top_k := pool (the same select work, the comparison), then
batch_search_exact_raw at top_k 10 with the training rows attached as f32 and as f16 (borrowed device tensors).  Recall@10 of the
estimate-only top 10 and of every exact leg against a flat exact search (torch.cdist over the f32 rows, top 10).
--pool-rule rank (profiles/bf_pool_rank/): every exact leg is timed under both pool rules, "heap"
(rbq_bf_search_exact_batch) and "rank" (rbq_bf_search_exact_ranked_batch), their windows alternating in one loop, with the recall of
each; the default, heap, is the run above."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bf_range_rate import windows  # noqa: E402  (the protocol: one copy)

TOP_K = 10


def kernel_table(a):
    """--kernel-table DIR: the brute-force kernels' device times from the *kernel_trace.csv files a `rocprofv3 --kernel-trace --stats
    -d DIR --` run of this tool (its own run, one window, one pool) left under DIR: per kernel the dispatches, their median and their
    sum in microseconds; for k_bf_rerank_score the raw-row bytes it requested (DIR/rate.json: calls x queries x pool x row bytes) over
    the sum of its times."""
    import csv
    import glob
    us = {}
    for f in glob.glob(os.path.join(a.kernel_table, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_bf_" in r["Kernel_Name"]:
                name = r["Kernel_Name"].split("(")[0].replace("void rbq::", "").replace("rbq::", "")
                us.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    run = json.load(open(os.path.join(a.kernel_table, "rate.json")))
    rec = {"source": "rocprofv3 --kernel-trace, a run of its own", "pools": run["pools"],
           "kernels": {k: {"dispatches": len(v), "median_us": round(statistics.median(v), 1), "sum_us": round(sum(v), 1)} for k, v in sorted(us.items())}}
    for raw, code in (("f32", 0), ("f16", 1)):
        k = rec["kernels"].get("k_bf_rerank_score<false, %d>" % code)
        if k:
            k["raw_bytes_requested"] = sum(len(run.get("pool_rules", ["heap"])) * run["exact_calls_per_leg"] * run["batch"] * p * run["dim"] * (4 if raw == "f32" else 2)
                                           for p in run["pools"])
            k["raw_TB_per_s"] = round(k["raw_bytes_requested"] / (k["sum_us"] * 1e-6) / 1e12, 3)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def alternating(fns, n_windows, calls):
    """tools.bf_range_rate.windows for several legs at once, their windows taking turns: {name: seconds per call}"""
    out = {name: [] for name in fns}
    for w in range(n_windows + 1):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            out[name].append((time.perf_counter() - t0) / calls)
    return {name: {"median_s": statistics.median(t[1:]), "min_s": min(t[1:]), "max_s": max(t[1:])} for name, t in out.items()}


def recall(ids, truth):
    return float(np.mean([len(set(ids[q].tolist()) & set(truth[q].tolist())) / TOP_K for q in range(len(truth))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--pools", type=int, nargs="+", default=[10, 100, 1024])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--pool-rule", choices=["heap", "rank"], default="heap", help="rank: time every exact leg under both pool rules, alternately")
    ap.add_argument("--kernel-table", default=None, metavar="DIR", help="no run: tabulate the kernel trace under DIR (see kernel_table)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.kernel_table:
        return kernel_table(a)
    import torch
    import rabitq_rs_amd as rq
    if not torch.cuda.is_available():
        sys.exit("bf_rerank_rate needs a GPU: nothing is measured without one")
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    x = torch.randn((a.n, a.dim), generator=g, device="cuda", dtype=torch.float32)
    idx = rq.BruteForceRabitqIndex.train_on_device(x, a.bits, 0, 1, a.seed, True)  # (L2, FHT-Kac rotator, faster config)
    rng = np.random.default_rng(a.seed)
    qt = torch.empty((a.batch, a.dim), dtype=torch.float32).pin_memory()
    qt.copy_(x[torch.from_numpy(rng.integers(0, a.n, a.batch)).cuda()].cpu() + 0.5 * torch.from_numpy(rng.standard_normal((a.batch, a.dim)).astype(np.float32)))
    q = qt.numpy()
    # (64 queries at a time: the direct kernel, no matrix product, was checked against |x|^2 - 2 q.x + |q|^2 at that size)
    truth = np.concatenate([torch.cdist(c, x, compute_mode="donot_use_mm_for_euclid_dist").topk(TOP_K, dim=1, largest=False).indices.cpu().numpy()
                            for c in qt.cuda().split(64)])
    p10 = rq.BruteForceSearchParams(TOP_K)
    rec = {"tool": "bf_rerank_rate", "n": a.n, "dim": a.dim, "bits": a.bits, "metric": "l2", "batch": a.batch, "top_k": TOP_K, "pools": a.pools,
           "windows": a.windows, "calls": a.calls, "exact_calls_per_leg": (a.windows + 1) * a.calls + 1,
           "pool_rules": ["heap", "rank"] if a.pool_rule == "rank" else ["heap"],
           "recall_at_10_estimate": recall(idx.batch_search_raw(q, p10)[0], truth)}
    stored = {"f32": x, "f16": x.half()}
    for pool in a.pools:
        rec["estimate_top_k_%d" % pool] = windows(lambda: idx.batch_search_raw(q, rq.BruteForceSearchParams(pool)), a.windows, a.calls)
        for raw, rows in stored.items():
            idx.set_rerank_vectors(rows)
            legs = alternating({r: (lambda r=r: idx.batch_search_exact_raw(q, p10, pool, pool_rule=r)) for r in rec["pool_rules"]}, a.windows, a.calls)
            for r, leg in legs.items():  # (one rule: the windows of tools.bf_range_rate.windows)
                leg["recall_at_10"] = recall(idx.batch_search_exact_raw(q, p10, pool, pool_rule=r)[0], truth)
                rec["exact_%s_pool_%d%s" % (raw, pool, "" if r == "heap" else "_rank")] = leg
            idx.set_rerank_vectors(None)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
