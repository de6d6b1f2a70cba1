"""Rate and host memory of the two RBQ1 loaders: IvfRabitqIndex.load_from_path (rbq_index_load_rbq1: the whole stream in one
host buffer, parsed and checksummed by one host thread) against IvfRabitqIndex.load_from_reader (rbq_index_load_rbq1_stream:
spans of at most 64 MB, checksummed and laid out by the GPU).

The parent process encodes an index on the GPU (default 2M x 960, 7-bit, 4096 lists, about 1.8 GB of RBQ1; random cluster
assignment, since only the size matters here), saves it to a file and leaves.  Each loader then runs in a child process of
its own, because a process's peak RSS never goes down: 5 loads of the file (page cache warm: it was just written, and a
warm-up read comes first), the median time, and the growth of the peak RSS (ru_maxrss) over what the process held before its
first load (taken after a small index went through both loaders, so that the runtime's first-use costs are not counted).
Writes profiles/load_rate_2m_d960.json (or --out) and prints it."""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(path, mode, runs):
    import torch
    import rabitq_rs_amd as rq
    torch.cuda.init()
    rq.index.lib()
    with open(path, "rb") as f:  # page cache
        while f.read(64 << 20):
            pass
    # first-use costs (the runtime's code objects, streams, the allocator's pools) are paid on a small index of the same
    # kind through both loaders, before the baseline: what is left is what a load of the file itself holds
    import io
    import numpy as np
    built = rq.builder.train(np.random.default_rng(1).random((2000, 64), dtype=np.float32), 16, 7, 0, 1, 1, True, kmeans_iters=2)
    small = bytes(built.save_rbq1())
    built.close()
    rq.IvfRabitqIndex.load_from_bytes(small).close()
    rq.IvfRabitqIndex.load_from_reader(io.BytesIO(small)).close()
    base = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    times, n = [], 0
    for _ in range(runs):
        t0 = time.perf_counter()
        if mode == "path":
            idx = rq.IvfRabitqIndex.load_from_path(path)
        else:
            with open(path, "rb", buffering=0) as f:
                idx = rq.IvfRabitqIndex.load_from_reader(f)
        times.append(time.perf_counter() - t0)
        n = len(idx)
        idx.close()
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    size = os.path.getsize(path)
    med = statistics.median(times)
    print(json.dumps({"loader": "load_from_path" if mode == "path" else "load_from_reader", "runs_s": times, "median_s": med,
                      "GB_per_s": size / med / 1e9, "vectors": n, "rss_before_kb": base, "peak_rss_kb": peak,
                      "peak_rss_growth_mb": (peak - base) / 1024.0}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory of the file written (default: the system temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load_rate_2m_d960.json"))
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--child", nargs=2, metavar=("PATH", "MODE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    fd, path = tempfile.mkstemp(suffix=".rbq", dir=a.dir)
    os.close(fd)
    try:
        # the build runs in a child too: this process never opens the GPU and holds nothing while the loaders run
        build = ("import sys, time, json, torch; sys.path.insert(0, %r); import rabitq_rs_amd as rq\n"
                 "n, dim, bits, nlist, seed, path = %d, %d, %d, %d, %d, %r\n"
                 "g = torch.Generator(device='cuda').manual_seed(seed)\n"
                 "x = torch.randn(n, dim, device='cuda', generator=g)\n"
                 "assign = torch.randint(0, nlist, (n,), device='cuda', generator=g)\n"
                 "assign[:nlist] = torch.arange(nlist, device='cuda')\n"
                 "cent = x[:nlist].cpu().numpy()\n"
                 "t0 = time.perf_counter(); idx = rq.IvfRabitqIndex.train_on_device(x, cent, assign, bits, 0, 1, seed, True)\n"
                 "t1 = time.perf_counter(); idx.save_to_path(path); t2 = time.perf_counter()\n"
                 "print(json.dumps({'encode_s': t1 - t0, 'save_s': t2 - t1}))\n"
                 % (ROOT, a.n, a.dim, a.bits, a.nlist, a.seed, path))
        out = {"n": a.n, "dim": a.dim, "bits": a.bits, "nlist": a.nlist, "runs": a.runs}
        out.update(json.loads(subprocess.run([sys.executable, "-c", build], check=True, capture_output=True, text=True,
                                             timeout=600).stdout.strip().splitlines()[-1]))
        out["file_bytes"] = os.path.getsize(path)
        for mode in ("path", "reader"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, mode, "--runs", str(a.runs)], check=True,
                               capture_output=True, text=True, timeout=900)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            out[res.pop("loader")] = res
    finally:
        os.unlink(path)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
