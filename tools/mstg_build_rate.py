"""Build time of MSTG posting lists: closure_assign (rbq_mstg_closure_assign) and build_postings_on_device
(rbq_mstg_build_device) against the CPU restatement plus the CPU builder.  N = 1 M vectors of dim 960, 1000 centroids
(every (N / 1000)-th row of the data, so that no leg needs a clustering step), 7 bits, L2, max_replicas 8.  Legs (--legs),
one process each so that every GPU step runs under a time limit of its own and nothing is started after a failure:

  timeout -k 10 300 python tools/mstg_build_rate.py --legs closure --out profiles/mstg_build_rate_1m_d960.json &&
  timeout -k 10 300 python tools/mstg_build_rate.py --legs build --out profiles/mstg_build_rate_1m_d960.json &&
  timeout -k 10 600 python tools/mstg_build_rate.py --legs cpu --out profiles/mstg_build_rate_1m_d960.json

(tools/mstg_build_rate.sh runs exactly that.)

  closure   closure_assign from a pageable host array and from a tensor already in HBM; replication factor, fallback rows
  build     build_postings_on_device (closure + grouping + encoder) from host and from HBM, rescale "optimal"
  cpu       closure_assign_cpu + builder.train_with_clusters over the expanded pairs on OMP_NUM_THREADS threads, over the
            first --cpu-n rows only (the whole set takes minutes).  It uses no GPU.  Its record says `scaled: true` and from how
            many rows: the *_scaled_to_n_s figures are the measured times times N / cpu_n (both steps are linear in N)

Every leg is the wall time of the whole call, one warm-up run and then the median of --repeats runs.  The data is a
Gaussian mixture in --intrinsic dimensions embedded in dim, so that vectors sit between clusters.  The closure leg checks
the device result against the CPU restatement on the first --check rows.  Each run merges its record into --out (JSON)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup=1):
    times = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if hasattr(out, "close"):
            out.close()
        if i >= warmup:
            times.append(dt)
    return {"median_s": round(float(np.median(times)), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4)}


def dataset(n, dim, intrinsic, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((64, intrinsic)).astype(np.float32)
    proj = rng.standard_normal((intrinsic, dim)).astype(np.float32) / np.float32(np.sqrt(intrinsic))
    x = np.empty((n, dim), np.float32)
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        low = means[rng.integers(0, 64, m)] + 0.35 * rng.standard_normal((m, intrinsic)).astype(np.float32)
        x[r0:r0 + m] = low @ proj + 0.02 * rng.standard_normal((m, dim)).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--epsilon", type=float, default=0.15)
    ap.add_argument("--max-replicas", type=int, default=8)
    ap.add_argument("--intrinsic", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=50000)
    ap.add_argument("--check", type=int, default=20000)
    ap.add_argument("--legs", default="closure,build,cpu")
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import rabitq_rs_amd as rq
    from rabitq_rs_amd import mstg
    legs = a.legs.split(",")
    if "closure" in legs or "build" in legs:
        import torch
        if not torch.cuda.is_available():
            sys.exit("the closure and build legs need a GPU: a CPU run says nothing about these times")
    data = dataset(a.n, a.dim, a.intrinsic, a.seed)
    cent = np.ascontiguousarray(data[:: a.n // a.lists][:a.lists])
    rec = {"tool": "mstg_build_rate", "n": a.n, "dim": a.dim, "lists": a.lists, "bits": a.bits, "metric": "l2", "epsilon": a.epsilon,
           "max_replicas": a.max_replicas, "intrinsic": a.intrinsic, "centroids": "every (n / lists)-th row", "repeats": a.repeats,
           "cpu_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0), "upload_bytes": int(data.nbytes)}
    eps, m = a.epsilon, a.max_replicas
    if "closure" in legs or "build" in legs:
        resident = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
    if "closure" in legs:
        before = mstg.closure_fallbacks()
        lists, counts = rq.closure_assign(resident, cent, eps, m)
        out = {"fallback_rows": mstg.closure_fallbacks() - before, "replication": round(float(counts.mean()), 4),
               "pairs": int(counts.sum())}
        want = rq.closure_assign_cpu(data[:a.check], cent, eps, m)
        out["equals_cpu_on_first_rows"] = bool(np.array_equal(lists[:a.check], want[0]) and np.array_equal(counts[:a.check], want[1]))
        out["device_from_host"] = timed(lambda: rq.closure_assign(data, cent, eps, m), a.repeats)
        out["device_from_resident"] = timed(lambda: rq.closure_assign(resident, cent, eps, m), a.repeats)
        rec["closure"] = out
    if "build" in legs:
        out = {}
        out["device_from_host"] = timed(lambda: rq.build_postings_on_device(data, cent, a.bits, 0, eps, m), a.repeats)
        out["device_from_resident"] = timed(lambda: rq.build_postings_on_device(resident, cent, a.bits, 0, eps, m), a.repeats)
        idx = rq.build_postings_on_device(resident, cent, a.bits, 0, eps, m)
        out["vectors_stored"] = len(idx)
        idx.close()
        rec["build"] = out
    if "cpu" in legs:
        sub = data[:a.cpu_n]
        out = {"rows": int(a.cpu_n), "scaled": True, "scaled_from_rows": int(a.cpu_n), "scaled_to_rows": a.n}
        out["closure"] = timed(lambda: rq.closure_assign_cpu(sub, cent, eps, m), 1, warmup=1)
        pv, pl = mstg.expand_pairs(*rq.closure_assign_cpu(sub, cent, eps, m))
        rows = sub[pv]
        out["builder"] = timed(lambda: rq.builder.train_with_clusters(rows, cent, pl, a.bits, 0, rq.RotatorType.NoRotation, 42, False), 1, warmup=0)
        scale = a.n / a.cpu_n
        out["closure_scaled_to_n_s"] = round(out["closure"]["median_s"] * scale, 2)
        out["build_scaled_to_n_s"] = round((out["closure"]["median_s"] + out["builder"]["median_s"]) * scale, 2)
        rec["cpu"] = out
    if a.out:
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old.update(rec)
        with open(a.out, "w") as f:
            f.write(json.dumps(old) + "\n")
    print(json.dumps(rec), flush=True)
    return 0 if rec.get("closure", {}).get("equals_cpu_on_first_rows", True) else 1


if __name__ == "__main__":
    sys.exit(main())
