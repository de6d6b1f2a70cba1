"""Time of the MSTG range search (rbq_mstg_range_batch*) next to the top-k search (rbq_mstg_search_batch*) on one handle: N = 1 M
vectors of dim 960, 7 bits, L2, batches of 1024 device-resident queries, the `balanced` preset (ef_search 150, pruning_epsilon
0.6), about 1000 lists.  The radius is the median over the batch of the --kth smallest estimate (--kth 100 is the shape to record),
so a query has about that many matches; the top-k leg runs at top_k = the median match count, which is what a caller without a
range search would have to guess.  One process per shape, under a time limit of its own, nothing started after a failure:

  timeout -k 10 900 python tools/mstg_range_rate.py --kth 100 --out profiles/mstg_range/rate_kth100.json

Every leg is a device-entry call timed between stream synchronisations: one warm-up window, then the median of --windows windows
of --calls calls each.  The same legs on the parent commit's library give the comparison for `mstg_search` (the range legs do not
exist there).  No rate has been recorded yet."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kth", type=int, default=100)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
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
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
