"""Wall time of MSTG's hierarchical balanced clustering: hierarchical_cluster (rbq_mstg_cluster_device) against (a) the CPU
restatement rbq_build_hcluster on OMP_NUM_THREADS threads and (b) what the library offered before: rbq_kmeans_device called
once per split from Python, the rows of every cluster gathered on the host.  Legs (--legs), one process each so that every GPU
step runs under a time limit of its own and nothing is started after a failure (tools/mstg_cluster_rate.sh runs them):

  device    hierarchical_cluster from a tensor already in HBM at --host-below: wall time, splits, host splits, clusters
  sweep     the same over --sweep values of host_below (the result must not change: checked)
  percall   baseline (b) over the first --percall-n rows: the stack walk in Python, run_kmeans_with_config per split
            (balancing left out: it moves at most 10 rows per split), scaled to N by N / percall_n
  cpu       baseline (a) over the first --cpu-n rows, scaled to N by N / cpu_n.  It uses no GPU.

Clustering cost grows a little faster than N (one more tree level per factor k), so both scaled figures flatter the
baselines; the records say `scaled: true` and from how many rows.  The data is the Gaussian mixture of
tools/mstg_build_rate.py.  Each run merges its record into --out (JSON) under the key --tag."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mstg_build_rate import dataset  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, round(time.perf_counter() - t0, 4)


def percall(rq, torch, x, mps, k, iters):
    """The stack walk with one rbq_kmeans_device call per split; returns the number of splits."""
    cfg = rq.KMeansConfig(niter=iters, nredo=1, seed=42, spherical=False, max_points_per_centroid=256, decode_block_size=32768)
    stack, splits, final = [np.arange(len(x))], 0, 0
    while stack:
        rows = stack.pop()
        if len(rows) <= mps:
            final += 1
            continue
        res = rq.run_kmeans_with_config(torch.from_numpy(x[rows]).cuda(), k, cfg)
        asg = res.assignments.cpu().numpy() if hasattr(res.assignments, "cpu") else np.asarray(res.assignments)
        splits += 1
        sub = [rows[asg == c] for c in range(k)]
        sub = [s for s in sub if len(s)]
        if len(sub) < 2:   # (no balancing here: halve instead of looping)
            sub = [rows[: len(rows) // 2], rows[len(rows) // 2:]]
        stack += sub
    return splits, final


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--max-posting-size", type=int, default=5000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--balance-weight", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-below", type=int, default=0)
    ap.add_argument("--sweep", default="0,1000,4000,16000,64000")
    ap.add_argument("--cpu-n", type=int, default=20000)
    ap.add_argument("--percall-n", type=int, default=100000)
    ap.add_argument("--intrinsic", type=int, default=8)
    ap.add_argument("--legs", default="device")
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import rabitq_rs_amd as rq
    legs = a.legs.split(",")
    gpu = any(leg in legs for leg in ("device", "sweep", "percall"))
    if gpu:
        import torch
        if not torch.cuda.is_available():
            sys.exit("the device, sweep and percall legs need a GPU: a CPU run says nothing about these times")
    data = dataset(a.n, a.dim, a.intrinsic, a.seed)
    mps, k, w, it = a.max_posting_size, a.k, a.balance_weight, a.iters
    rec = {"tool": "mstg_cluster_rate", "n": a.n, "dim": a.dim, "max_posting_size": mps, "branching_factor": k, "balance_weight": w,
           "max_iterations": it, "intrinsic": a.intrinsic, "cpu_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}
    if gpu:
        resident = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        rq.hierarchical_cluster(resident[:4096], 512, k, w, 2)  # warm-up: module load

    def run(hb):
        (cent, off, mem, st), t = wall(lambda: rq.hierarchical_cluster(resident, mps, k, w, it, host_below=hb))
        return {"host_below": hb, "wall_s": t, "clusters": int(len(off) - 1), **st}, (cent, off, mem)

    if "device" in legs:
        rec["device"], _ = run(a.host_below)
    if "sweep" in legs:
        out, first, same = [], None, True
        for hb in (int(v) for v in a.sweep.split(",")):
            r, arrays = run(hb)
            out.append(r)
            if first is None:
                first = arrays
            else:
                same = same and all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(first, arrays))
        rec["sweep"] = {"runs": out, "results_identical": bool(same), "best_host_below": min(out, key=lambda r: r["wall_s"])["host_below"]}
    if "percall" in legs:
        sub = data[:a.percall_n]
        percall(rq, torch, sub[:4096], 512, k, 2)
        (splits, final), t = wall(lambda: percall(rq, torch, sub, mps, k, it))
        rec["percall"] = {"rows": a.percall_n, "wall_s": t, "splits": splits, "clusters": final, "scaled": True,
                          "scaled_from_rows": a.percall_n, "scaled_to_rows": a.n, "scaled_to_n_s": round(t * a.n / a.percall_n, 2)}
    if "cpu" in legs:
        sub = data[:a.cpu_n]
        (_, off, _, st), t = wall(lambda: rq.hierarchical_cluster_cpu(sub, mps, k, w, it))
        rec["cpu"] = {"rows": a.cpu_n, "wall_s": t, "clusters": int(len(off) - 1), **st, "scaled": True, "scaled_from_rows": a.cpu_n,
                      "scaled_to_rows": a.n, "scaled_to_n_s": round(t * a.n / a.cpu_n, 2)}
    if a.out:
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old.setdefault(a.tag, {}).update(rec)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(old) + "\n")
    print(json.dumps(rec), flush=True)
    return 0 if rec.get("sweep", {}).get("results_identical", True) else 1


if __name__ == "__main__":
    sys.exit(main())
