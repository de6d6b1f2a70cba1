"""Rate of rbq_index_fetch_embeddings (include/rbq.h; the crate's fetch_embedding): 1 M random ids fetched from a GIST-1M-shaped
index (default 1M x 960, FHT-Kac, 7-bit, 4096 lists) and from Matrix-rotator indexes (d = 128 and 960), through the host entry
and the device entry.  The first fetch of each handle (the id map build) is timed on its own.  The indexes are encoded on the GPU
over random assignments (the rate does not depend on the clustering).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_index(n, dim, bits, nlist, rot, seed):
    import torch
    import rabitq_rs_amd as rq
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, dim, device="cuda", generator=g)
    assign = torch.randint(0, nlist, (n,), device="cuda", generator=g, dtype=torch.int64)
    cent = x[:nlist].cpu().numpy()
    idx = rq.IvfRabitqIndex.train_on_device(x, cent, assign, bits, 0, rot, seed, True)
    del x, assign
    torch.cuda.empty_cache()
    return idx


def rate(idx, n, nq, reps, seed):
    import torch
    out = {}
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    idx.fetch_embeddings([0])  # first call of the handle: builds the id map
    out["first_call_s"] = time.perf_counter() - t0
    q = rng.integers(0, n, nq).astype(np.uint64)
    idx.fetch_embeddings(q)  # warm-up (pinned buffers, kernels)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, found = idx.fetch_embeddings(q)
        ts.append(time.perf_counter() - t0)
    assert found.all()
    out["host_s"] = min(ts)
    out["host_ids_per_s"] = nq / min(ts)
    d_ids = torch.from_numpy(q.view(np.int64)).cuda()
    d_out = torch.empty((nq, idx.dim), dtype=torch.float32, device="cuda")
    d_found = torch.empty(nq, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    idx.fetch_embeddings_device(d_ids.data_ptr(), nq, d_out.data_ptr(), d_found.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(s)
        idx.fetch_embeddings_device(d_ids.data_ptr(), nq, d_out.data_ptr(), d_found.data_ptr(), s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out["device_ms"] = min(ms)
    out["device_ids_per_s"] = nq / (min(ms) / 1e3)
    out["device_out_GB_per_s"] = nq * idx.dim * 4 / (min(ms) / 1e3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--matrix-dims", default="128,960")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261015)
    a = ap.parse_args()
    res = {"n": a.n, "nq": a.nq, "bits": a.bits, "nlist": a.nlist}
    idx = make_index(a.n, a.dim, a.bits, a.nlist, 1, a.seed)
    res["fhtkac_%d" % a.dim] = rate(idx, a.n, a.nq, a.reps, a.seed)
    idx.close()
    for d in (int(v) for v in a.matrix_dims.split(",") if v):
        idx = make_index(a.n, d, a.bits, a.nlist, 0, a.seed + d)
        res["matrix_%d" % d] = rate(idx, a.n, a.nq, a.reps, a.seed)
        idx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
