"""Build rate of the GPU encoder, constant (RabitqConfig::faster) against optimal rescale (RabitqConfig::new), and of the CPU
builder for comparison.  One measurement per process, so that every call can run under its own time limit:

  --mode const | optimal   rbq_index_build_device_ex over N vectors resident on the GPU (one warm-up build, then the timed one)
  --mode stream            the streamed optimal build (rbq_build_stream_*), host chunks of --chunk vectors
  --mode cpu_const | cpu_optimal   the CPU builder (train_with_clusters, OpenMP) on N vectors

Data: a Gaussian mixture generated on the GPU, --nlist clusters assigned by nearest centroid.  Prints one JSON line with
vectors per second (wall time of the build call, host overheads included)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_data(torch, n, dim, nlist, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    means = torch.randn(64, dim, device="cuda", generator=g)
    x = torch.empty(n, dim, device="cuda")
    step = 1 << 16
    for s in range(0, n, step):
        e = min(n, s + step)
        comp = torch.randint(0, 64, (e - s,), device="cuda", generator=g)
        x[s:e] = means[comp] + 0.35 * torch.randn(e - s, dim, device="cuda", generator=g)
    cent = x[torch.randperm(n, device="cuda", generator=g)[:nlist]].clone()
    assign = torch.empty(n, dtype=torch.int32, device="cuda")
    c2 = (cent * cent).sum(1)
    for s in range(0, n, step):
        e = min(n, s + step)
        assign[s:e] = (c2[None, :] - 2.0 * x[s:e] @ cent.T).argmin(1).to(torch.int32)
    return x, cent, assign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["const", "optimal", "stream", "cpu_const", "cpu_optimal"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=20261015)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    x, cent, assign = make_data(torch, a.n, a.dim, a.nlist, a.seed)
    cent_h = cent.cpu().numpy()
    rec = {"tool": "encode_rate", "mode": a.mode, "n": a.n, "dim": a.dim, "bits": a.bits, "nlist": a.nlist}
    if a.mode.startswith("cpu"):
        xh, ah = x.cpu().numpy(), assign.cpu().numpy().astype(np.uint32)
        del x
        t0 = time.perf_counter()
        b = rq.builder.train_with_clusters(xh, cent_h, ah, a.bits, 0, 1, a.seed, a.mode == "cpu_const")
        dt = time.perf_counter() - t0
        b.close()
        rec["threads"] = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    else:
        small = rq.builder.train_with_clusters(x[:a.nlist].cpu().numpy(), cent_h, np.arange(a.nlist, dtype=np.uint32), a.bits,
                                               0, 1, a.seed, True)
        t_const = small.t_const
        if a.mode == "stream":
            sizes = torch.bincount(assign.long(), minlength=a.nlist).cpu().numpy().astype(np.uint32)
            xh, ah = x.cpu().numpy(), assign.cpu().numpy().astype(np.uint32)
            del x
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sb = rq.StreamBuilder(small.hdr_ptr, cent_h, sizes, None, rescale="optimal")
            for s in range(0, a.n, a.chunk):
                sb.push(xh[s:s + a.chunk], ah[s:s + a.chunk], s)
            idx = sb.finish()
            dt = time.perf_counter() - t0
            rec["chunk"] = a.chunk
        else:
            build = lambda: rq.IvfRabitqIndex.build_on_device(small.hdr_ptr, cent_h, x.data_ptr(), assign.data_ptr(), a.n,  # noqa: E731
                                                               t_const, rescale=a.mode)
            build().close()  # warm-up (code objects, allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx = build()
            dt = time.perf_counter() - t0
        assert len(idx) == a.n
        idx.close()
    rec.update({"seconds": round(dt, 4), "vectors_per_s": round(a.n / dt, 1)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
