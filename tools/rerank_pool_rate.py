"""Recall and rate of the pooled rerank (option "rerank_pool") on the benchmark's data: N = 1 M vectors of dim
960 (bench.py's GIST-1M-shaped mixture), nlist 4096, 7 bits, L2, one batch of 1024 device-resident queries, top_k = 10,
nprobe 32 and 128, pool off / 32 / 64 / 128 / 256 / 1024.  The raw vectors stay on the device and are attached as a borrowed pointer.

  timeout -k 10 900 python tools/rerank_pool_rate.py --out profiles/rerank_pool/rate.json
  timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rerank_pool_rate.py --traced --out DIR/traced.json
  python tools/rerank_pool_rate.py --kernel-table DIR --rate profiles/rerank_pool/rate.json --out profiles/rerank_pool/kernels.json

Per configuration: recall@10 against the exact top 10 (float64 on the GPU), and queries/s — the wall time of --calls calls of
rbq_search_batch_device on one stream between two synchronisations, one warm-up window per configuration, then --rounds rounds
that visit every configuration in turn; the median of the rounds is reported next to their spread.
The yardstick for a pool p <= 1024 is what the library could do before the option existed: the search at top_k := p with the
rerank on (k_rerank over p ids), of which the caller keeps the first 10 — the `sliced` legs, timed in the same rounds.
--traced runs every leg a fixed number of times with no timing (for a kernel trace of its own); --kernel-table reads that trace:
the two rerank kernels' dispatches are assigned to their legs by their order (the legs run one after the other, each a fixed
number of calls), and each is reported as requested bytes (sum of counts x dim x element size) over kernel time.
--raw-dtype f32 f16 bf16 (any of them): the element type the attached rows are kept in.  For f16 / bf16 the
benchmark's rows are rounded once on the device (round to nearest even) and that copy is borrowed; recall stays against the float64
exact top 10 of the UNROUNDED rows.  With several types every round visits every leg of every type in turn (names of legs other
than f32's end in _f16 / _bf16), so the types are measured beside each other; --pools / --nprobes restrict the legs."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOLS = (32, 64, 128, 256, 1024)
NPROBES = (32, 128)
HBM_PEAK_TBS = 8.0       # MI355X HBM3E, specification
HBM_MEASURED_TBS = 6.29  # float4 copy


def exact_topk_f64(torch, x, q, k):
    """ids of the k smallest squared distances per query, float64, over chunks of the base vectors"""
    q64 = q.double()
    qn = (q64 * q64).sum(1, keepdim=True)
    bv = torch.full((q.shape[0], k), float("inf"), dtype=torch.float64, device=q.device)
    bi = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=q.device)
    for s in range(0, x.shape[0], 65536):
        xc = x[s:s + 65536].double()
        d = qn - 2.0 * (q64 @ xc.T) + (xc * xc).sum(1)[None, :]
        v, i = d.topk(min(k, xc.shape[0]), dim=1, largest=False)
        cv, ci = torch.cat([bv, v], 1), torch.cat([bi, i + s], 1)
        bv, si = cv.topk(k, dim=1, largest=False)
        bi = torch.gather(ci, 1, si)
    return bi


ELEM_BYTES = {"f32": 4, "f16": 2, "bf16": 2}


def legs(a):
    """(name, nprobe, rerank, pool option, top_k of the call, raw dtype)"""
    out = []
    for nprobe in a.nprobes:
        out.append((f"np{nprobe}_off", nprobe, 0, 0, 10, a.raw_dtype[0]))
        for dt in a.raw_dtype:
            sfx = "" if dt == "f32" else "_" + dt
            out.append((f"np{nprobe}_rerank_unpooled{sfx}", nprobe, 1, 0, 10, dt))
            for p in a.pools:
                out.append((f"np{nprobe}_pool{p}{sfx}", nprobe, 1, p, 10, dt))
                out.append((f"np{nprobe}_sliced{p}{sfx}", nprobe, 1, 0, p, dt))
    return out


def kernel_table(a):
    rate = json.load(open(a.rate))
    dim, traced = rate["dim"], json.load(open(os.path.join(a.kernel_table, "traced.json")))
    n = traced["calls_per_leg"]
    rows = []
    for f in glob.glob(os.path.join(a.kernel_table, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    pooled = [r for r in rows if "k_rerank_pool" in r["Kernel_Name"]]
    plain = [r for r in rows if "k_rerank" in r["Kernel_Name"] and "k_rerank_pool" not in r["Kernel_Name"]]
    # the order of legs(): every leg with the rerank on dispatches one rerank kernel per call, k_rerank_pool where its pool exceeds
    # its top_k and k_rerank otherwise
    a.raw_dtype, a.pools, a.nprobes = traced.get("raw_dtype", ["f32"]), traced.get("pools", list(POOLS)), traced.get("nprobes", list(NPROBES))
    L = [leg for leg in legs(a) if leg[2]]
    want_pooled = n * sum(1 for leg in L if leg[3] > leg[4])
    if len(pooled) != want_pooled or len(plain) != n * len(L) - want_pooled:
        raise SystemExit(f"unexpected dispatch counts: k_rerank_pool {len(pooled)}, k_rerank {len(plain)}")
    rec = {"source": "rocprofv3 --kernel-trace, a run of its own", "calls_per_leg": n,
           "hbm_peak_TBps": HBM_PEAK_TBS, "hbm_measured_copy_TBps": HBM_MEASURED_TBS, "kernels": {}}
    for name, nprobe, _, pool, k, dt in L:
        src = pooled if pool > k else plain
        d, src[:] = src[:n], src[n:]
        if not pool and k == 10:
            continue  # (the unpooled rerank of the answer itself: ten rows per query, not a rate)
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in d]
        assert all(("k_rerank_pool" in r["Kernel_Name"]) == (pool > k) for r in d)
        entries = next(v["pool_entries"] for nm, v in rate["legs"].items() if nm.split("_")[:2] == [f"np{nprobe}", f"pool{pool or k}"])
        req = entries * dim * ELEM_BYTES[dt]  # (the pool's entries do not depend on the type the rows are kept in)
        med = statistics.median(us)
        rec["kernels"][name] = {"kernel": d[0]["Kernel_Name"], "raw_dtype": dt, "dispatches": len(us),
                                "median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                                "requested_bytes": req, "requested_TBps": round(req / (med * 1e-6) / 1e12, 3)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--raw-dtype", nargs="+", choices=("f32", "f16", "bf16"), default=["f32"])
    ap.add_argument("--pools", nargs="+", type=int, default=list(POOLS))
    ap.add_argument("--nprobes", nargs="+", type=int, default=list(NPROBES))
    ap.add_argument("--traced", action="store_true")
    ap.add_argument("--kernel-table", default=None, metavar="DIR")
    ap.add_argument("--rate", default=None)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.kernel_table:
        return kernel_table(a)
    import torch
    import bench
    import rabitq_rs_amd as rq
    dev = torch.device("cuda", 0)
    top_k = 10
    mix = bench.Mixture(torch, dev, a.dim, a.nlist, "mixture_id32", False)
    q = mix.draw(a.batch, 20260102).contiguous()
    x = mix.draw(a.n, 20260105)
    cent, assign = bench.kmeans_gpu(torch, x, a.nlist, 6, 20260103)
    cent_h = cent.cpu().numpy()
    ns = max(2 * a.nlist, 4096)  # (the header — rotator, t_const — from a CPU build over a tiny subset, as bench.py --device-build takes it)
    small = rq.builder.train_with_clusters(mix.draw(ns, 99).cpu().numpy(), cent_h, (np.arange(ns) % a.nlist).astype(np.uint32), 7, 0,
                                           rq.RotatorType.FhtKacRotator, 20260104, True)
    a32 = assign.to(torch.int32).contiguous()
    idx = rq.IvfRabitqIndex.build_on_device(small.hdr_ptr, cent_h, x.data_ptr(), a32.data_ptr(), a.n, small.t_const, device=0)
    rows = {"f32": x}  # what each type's legs borrow; 16-bit: the rows rounded once (to nearest even), as a caller would keep them
    for dt in a.raw_dtype:
        if dt != "f32":
            rows[dt] = x.to(torch.float16 if dt == "f16" else torch.bfloat16).contiguous()
    attached = [None]
    gt = None if a.traced else exact_topk_f64(torch, x, q, top_k).cpu().numpy()
    st = torch.cuda.Stream(dev)
    bufs = {}

    def run(leg, calls):
        _, nprobe, rerank, pool, k, dt = leg
        if attached[0] != dt:  # (outside the timed window)
            idx.set_rerank_vectors(device_ptr=rows[dt].data_ptr(), n=a.n, **({} if dt == "f32" else {"dtype": dt}))
            attached[0] = dt
        if k not in bufs:
            bufs[k] = (torch.zeros(a.batch, k, dtype=torch.int64, device=dev), torch.zeros(a.batch, k, dtype=torch.float32, device=dev),
                       torch.zeros(a.batch, dtype=torch.int32, device=dev))
        d_i, d_s, d_c = bufs[k]
        idx.set_option("rerank", rerank)
        idx.set_rerank_pool(pool)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            idx.search_batch_device(q.data_ptr(), a.batch, a.dim, k, nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, d_i, d_c

    rec = {"n": a.n, "dim": a.dim, "nlist": a.nlist, "bits": 7, "metric": "L2", "batch": a.batch, "top_k": top_k, "dataset": "mixture_id32",
           "calls_per_window": a.calls, "rounds": a.rounds, "legs": {}}
    rec.update({"raw_dtype": a.raw_dtype, "pools": a.pools, "nprobes": a.nprobes})
    L = legs(a)
    if a.traced:
        rec = {"calls_per_leg": 6, "raw_dtype": a.raw_dtype, "pools": a.pools, "nprobes": a.nprobes}
        for leg in L:
            run(leg, rec["calls_per_leg"])
    else:
        for leg in L:  # warm-up of every shape, and the results
            _, d_i, d_c = run(leg, 3)
            ids = d_i.cpu().numpy()[:, :top_k]
            r = {"recall_at_10": round(bench.recall_of(ids, gt, top_k), 4), "mean_count": float(d_c.float().mean())}
            if leg[3]:  # entries of the pools: what the plain search at top_k := pool returns
                _, _, p_c = run((None, leg[1], 0, 0, leg[3], leg[5]), 1)
                r["pool_entries"] = int(p_c.sum())
            rec["legs"][leg[0]] = r
        times = {leg[0]: [] for leg in L}
        for _ in range(a.rounds):
            for leg in L:
                times[leg[0]].append(run(leg, a.calls)[0])
        for name, ts in times.items():
            qps = sorted(a.batch * a.calls / t for t in ts)
            rec["legs"][name].update({"queries_per_s_median": round(statistics.median(qps)), "queries_per_s_min": round(qps[0]),
                                      "queries_per_s_max": round(qps[-1]), "ms_per_call_median": round(1e3 * statistics.median(ts) / a.calls, 4)})
    idx.release_stream(st.cuda_stream)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
