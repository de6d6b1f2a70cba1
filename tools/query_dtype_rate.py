"""Rate of the search with f16 / bf16 queries (option "query_dtype") on the benchmark's data: N = 1 M vectors of
dim 960 (bench.py's GIST-1M-shaped mixture), nlist 4096, 7 bits, L2, top_k 10, nprobe 128.

  timeout -k 10 1100 python tools/query_dtype_rate.py --out profiles/query_dtype/rate.json

Legs (the protocol of tools/range_rate.py: the wall time of a window of --calls calls between two synchronisations, one warm-up
window, then --rounds rounds that visit every leg in turn; medians with min - max beside them):
  * the host call (rbq_search_batch through the C ABI, results into page-locked arrays, the option set once per leg) at 1, 64, 256,
    1024 and 4096 queries per call, queries page-locked and pageable, f32 / f16 / bf16;
  * the device entry (rbq_search_batch_device on one stream) at --batch queries for the three types;
  * the device entry for f16 input as a caller serves it without the option: torch's .float() into a scratch tensor, then the f32 call;
  * `_offset` legs: the f16 rows one element into a larger buffer, so every row starts 2-byte aligned only and the preparation takes
    one 16-bit load per element instead of the paired 32-bit loads (page-locked host legs and the device entry).
The reference of a 16-bit leg is the f32 leg of the same run: `ratio_to_f32` = its median time per call over the f32 leg's, with the
bytes of queries a call moves beside it.  The 16-bit queries are the f32 ones rounded once; results are not compared here (the tests do)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = ("f32", "f16", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=128)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024, help="queries per call of the device-entry legs")
    ap.add_argument("--host-nq", nargs="+", type=int, default=[1, 64, 256, 1024, 4096])
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import bench
    import rabitq_rs_amd as rq
    dev = torch.device("cuda", 0)
    mix = bench.Mixture(torch, dev, a.dim, a.nlist, "mixture_id32", False)
    nq_max = max(a.host_nq + [a.batch])
    q = mix.draw(nq_max, 20260102).contiguous()
    x = mix.draw(a.n, 20260105)
    cent, assign = bench.kmeans_gpu(torch, x, a.nlist, 6, 20260103)
    cent_h = cent.cpu().numpy()
    ns = max(2 * a.nlist, 4096)  # (the header — rotator, t_const — from a CPU build over a tiny subset, as bench.py --device-build takes it)
    small = rq.builder.train_with_clusters(mix.draw(ns, 99).cpu().numpy(), cent_h, (np.arange(ns) % a.nlist).astype(np.uint32), 7, 0,
                                           rq.RotatorType.FhtKacRotator, 20260104, True)
    a32 = assign.to(torch.int32).contiguous()
    idx = rq.IvfRabitqIndex.build_on_device(small.hdr_ptr, cent_h, x.data_ptr(), a32.data_ptr(), a.n, small.t_const, device=0)
    del x
    L = rq.index.lib()
    tt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    dq = {t: q.to(tt[t]).contiguous() for t in TYPES}                      # device
    hq = {t: dq[t].cpu().contiguous() for t in TYPES}                      # pageable host
    pq = {t: hq[t].pin_memory() for t in TYPES}                            # page-locked host
    def one_in(t16):  # the same rows one element into a larger buffer of the same memory kind
        flat = torch.zeros(t16.numel() + 1, dtype=t16.dtype, device=t16.device)
        flat = flat.pin_memory() if t16.is_pinned() else flat
        flat[1:] = t16.reshape(-1)
        out = flat[1:].view(t16.shape)
        assert out.data_ptr() % 4 == 2
        return out
    dq["f16_offset"], pq["f16_offset"] = one_in(dq["f16"]), one_in(pq["f16"])
    o_i = torch.zeros(nq_max, a.top_k, dtype=torch.int64).pin_memory()
    o_s = torch.zeros(nq_max, a.top_k, dtype=torch.float32).pin_memory()
    o_c = torch.zeros(nq_max, dtype=torch.int32).pin_memory()
    d_i = torch.zeros(a.batch, a.top_k, dtype=torch.int64, device=dev)
    d_s = torch.zeros(a.batch, a.top_k, dtype=torch.float32, device=dev)
    d_c = torch.zeros(a.batch, dtype=torch.int32, device=dev)
    scratch = torch.empty(a.batch, a.dim, dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(dev)

    def host_leg(t, nq, src):
        def run(calls):
            idx.set_query_dtype(t.split("_")[0])
            p = src[t].data_ptr()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(calls):
                rc = L.rbq_search_batch(idx._h, p, nq, a.dim, a.top_k, a.nprobe, None, 0, o_i.data_ptr(), o_s.data_ptr(), o_c.data_ptr(), None)
            dt = time.perf_counter() - t0
            idx.set_query_dtype(None)
            assert rc == 0, rq.index._detail()
            return dt
        return run

    def device_leg(t, widen_first):
        def run(calls):
            idx.set_query_dtype("f32" if widen_first else t.split("_")[0])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.cuda.stream(st):
                for _ in range(calls):
                    src = dq[t][:a.batch]
                    if widen_first:  # what a caller does without the option: a widening kernel of its own into a second buffer
                        scratch.copy_(src)
                        src = scratch
                    idx.search_batch_device(src.data_ptr(), a.batch, a.dim, a.top_k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(),
                                            stream=st.cuda_stream)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            idx.set_query_dtype(None)
            return dt
        return run

    legs = {}
    for nq in a.host_nq:
        for mem, src in (("pinned", pq), ("pageable", hq)):
            for t in TYPES:
                legs[f"host_{mem}_nq{nq}_{t}"] = (host_leg(t, nq, src), nq, t, f"host_{mem}_nq{nq}_f32", "h2d")
        legs[f"host_pinned_nq{nq}_f16_offset"] = (host_leg("f16_offset", nq, pq), nq, "f16", f"host_pinned_nq{nq}_f32", "h2d")
    for t in TYPES + ("f16_offset",):
        legs[f"device_nq{a.batch}_{t}"] = (device_leg(t, False), a.batch, t.split("_")[0], f"device_nq{a.batch}_f32", "none")
    legs[f"device_nq{a.batch}_f16_widened_by_caller"] = (device_leg("f16", True), a.batch, "f16", f"device_nq{a.batch}_f32", "none")
    rec = {"n": a.n, "dim": a.dim, "nlist": a.nlist, "bits": 7, "metric": "L2", "top_k": a.top_k, "nprobe": a.nprobe, "dataset": "mixture_id32",
           "calls_per_window": a.calls, "rounds": a.rounds, "legs": {}}
    for name, (run, nq, t, ref, _) in legs.items():
        run(2)        # (the first call sizes the workspace)
        run(a.calls)  # warm-up window
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, (run, nq, t, ref, _) in legs.items():
            times[name].append(run(a.calls) / a.calls)
    for name, (run, nq, t, ref, moved) in legs.items():
        ts = sorted(times[name])
        rec["legs"][name] = {"queries_per_call": nq, "query_dtype": t,
                             "query_bytes_per_call": nq * a.dim * (4 if t == "f32" else 2), "rows_2_byte_aligned_only": name.endswith("_offset"), "travel": moved,
                             "us_per_call_median": round(1e6 * statistics.median(ts), 2), "us_per_call_min": round(1e6 * ts[0], 2),
                             "us_per_call_max": round(1e6 * ts[-1], 2), "queries_per_s_median": round(nq / statistics.median(ts))}
    for name, (run, nq, t, ref, _) in legs.items():
        rec["legs"][name]["ratio_to_f32"] = round(rec["legs"][name]["us_per_call_median"] / rec["legs"][ref]["us_per_call_median"], 4)
    idx.release_stream(st.cuda_stream)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
