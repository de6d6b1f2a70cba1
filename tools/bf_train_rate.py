"""Training time of the brute-force index: BruteForceRabitqIndex.train_on_device (rbq_bf_train_device) against the CPU builder.
N = 200 000 vectors of dim 1024 (the size the crate's doc comment names as this index's use case), 7 bits, L2, FhtKac, for both
rescale modes (const = RabitqConfig::faster, optimal = RabitqConfig::new).  Three legs per mode:

  device_from_host      train_on_device from a pageable host array: upload, rotation, quantisation, packing
  device_from_resident  train_on_device from a tensor already in HBM
  cpu_builder           builder.train_bruteforce (OpenMP, OMP_NUM_THREADS threads); the upload that `train` adds is not included

Every leg is the wall time of the whole call (the device calls end in a device synchronise), one warm-up run and then the
median of --repeats runs.  One index of each route is saved and the two streams compared, so a run also shows that the times
belong to equal results.  Prints one JSON line."""
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
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=5)
    ap.add_argument("--modes", default="const,optimal")
    ap.add_argument("--seed", type=int, default=20261017)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    if not torch.cuda.is_available():
        sys.exit("bf_train_rate needs a GPU: a CPU run says nothing about these times")
    BF, FHT, L2 = rq.BruteForceRabitqIndex, rq.RotatorType.FhtKacRotator, rq.Metric.L2
    data = np.random.default_rng(a.seed).standard_normal((a.n, a.dim)).astype(np.float32)
    resident = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    rec = {"tool": "bf_train_rate", "n": a.n, "dim": a.dim, "bits": a.bits, "rotator": "fht_kac", "metric": "l2",
           "repeats": a.repeats, "cpu_repeats": a.cpu_repeats, "cpu_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
           "upload_bytes": int(data.nbytes), "modes": {}}
    for mode in a.modes.split(","):
        faster = mode == "const"
        legs = {"device_from_host": (lambda: BF.train_on_device(data, a.bits, L2, FHT, a.seed, faster), a.repeats),
                "device_from_resident": (lambda: BF.train_on_device(resident, a.bits, L2, FHT, a.seed, faster), a.repeats),
                "cpu_builder": (lambda: rq.builder.train_bruteforce(data, a.bits, L2, FHT, a.seed, faster), a.cpu_repeats)}
        out = {}
        for name, (fn, reps) in legs.items():
            med, lo, hi = timed(fn, reps)
            print("%s %s: median %.3f s" % (mode, name, med), file=sys.stderr, flush=True)
            out[name] = {"median_s": round(med, 4), "min_s": round(lo, 4), "max_s": round(hi, 4),
                         "vectors_per_s": round(a.n / med, 1)}
        dev = BF.train_on_device(resident, a.bits, L2, FHT, a.seed, faster)
        built = rq.builder.train_bruteforce(data, a.bits, L2, FHT, a.seed, faster)
        cpu = BF.from_built(built)
        out["streams_equal"] = dev.save_to_bytes() == cpu.save_to_bytes()
        for x in (dev, cpu, built):
            x.close()
        out["host_over_cpu"] = round(out["device_from_host"]["median_s"] / out["cpu_builder"]["median_s"], 4)
        out["resident_over_cpu"] = round(out["device_from_resident"]["median_s"] / out["cpu_builder"]["median_s"], 4)
        rec["modes"][mode] = out
    print(json.dumps(rec), flush=True)
    return 0 if all(m["streams_equal"] for m in rec["modes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
