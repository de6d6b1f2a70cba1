"""Rate of the device k-means (run_kmeans_with_config, k_kmeans.hip) and of its CPU restatement for comparison.  One
measurement per process, so that every call can run under its own time limit:

  --mode gpu   rbq_kmeans_device over N vectors resident on the GPU (one warm-up run on a small subset, then the timed run)
  --mode cpu   the CPU restatement (rbq_build_kmeans_faiss, OpenMP) on N vectors

Data: a Gaussian mixture generated on the GPU (64 components).  Prints one JSON line: wall time of the k-means call (host
overheads included), the nominal assignment work 2 N' k d per pass over (niter passes over the training rows N', one over all
N rows) and the rate that work implies over the whole call."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_data(torch, n, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    means = torch.randn(64, dim, device="cuda", generator=g)
    x = torch.empty(n, dim, device="cuda")
    step = 1 << 16
    for s in range(0, n, step):
        e = min(n, s + step)
        comp = torch.randint(0, 64, (e - s,), device="cuda", generator=g)
        x[s:e] = means[comp] + 0.35 * torch.randn(e - s, dim, device="cuda", generator=g)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["gpu", "cpu"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--niter", type=int, default=30)
    ap.add_argument("--mppc", type=int, default=256)
    ap.add_argument("--seed", type=int, default=20261015)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    cfg = rq.KMeansConfig(niter=a.niter, seed=a.seed, max_points_per_centroid=a.mppc)
    x = make_data(torch, a.n, a.dim, a.seed)
    rec = {"tool": "kmeans_rate", "mode": a.mode, "n": a.n, "dim": a.dim, "k": a.k, "niter": a.niter}
    st = {}
    if a.mode == "cpu":
        xh = x.cpu().numpy()
        del x
        t0 = time.perf_counter()
        res = rq.builder.run_kmeans_with_config_cpu(xh, a.k, cfg, stats=st)
        dt = time.perf_counter() - t0
        rec["threads"] = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    else:
        warm = min(a.n, max(a.k, 20000))
        rq.run_kmeans_with_config(x[:warm], a.k, rq.KMeansConfig(niter=1, seed=a.seed))  # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = rq.run_kmeans_with_config(x, a.k, cfg, stats=st)
        dt = time.perf_counter() - t0
    rows = max(min(a.n, a.k * a.mppc), a.k)
    flop = 2.0 * a.k * a.dim * (a.niter * rows + a.n)
    rec.update({"seconds": round(dt, 4), "train_rows": rows, "assign_tflop": round(flop / 1e12, 2),
                "implied_tflops": round(flop / dt / 1e12, 2), "objective": res.objective, **st})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
