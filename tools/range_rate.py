"""Rate of the range search (options "range_search" / "range_radius_bits") on the benchmark's data: N = 1 M
vectors of dim 960 (bench.py's GIST-1M-shaped mixture), nlist 4096, 7 bits, L2, nprobe 128, batches of 1024 device-resident queries.

  timeout -k 10 900 python tools/range_rate.py --out profiles/range_search/rate.json

The radii are the medians, over the batch, of the 10th, 100th and 1000th distance of the top-k search at top_k = 1000.  Per radius:
  * the range search at a capacity that truncates nothing (the largest total of the batch, read from a first call), and
  * the only way to get those sets before the option existed: rbq_search_batch_device at top_k := that capacity, option off (the
    top-k path of this library is the parent's: the option does not touch it),
each as queries/s — the wall time of a window of calls on one stream between two synchronisations, one warm-up window, then --rounds
rounds that visit every leg in turn; medians with the spread — and as the time of the scan stage (k_range, or the top-k scan) from
the library's own stage profile (event pairs around the kernel), in a pass of its own.  A window holds --calls calls, fewer for a
leg whose single call takes longer than --window-s / --calls (the top-k scan at a large top_k); never fewer than two.
The comparison is not tuned: both legs run with the library's defaults."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def exact_legs(a, torch, dev, idx, x_rows, q, st):
    """--exact: the exact range search (options "range_exact" / "range_exact_radius_bits") on the same index and batch.
    x is the batch's median 10th / 100th EXACT neighbour distance (the pooled rerank at top_k 100, pool 1024, over the probed lists);
    the candidate radius r is x, 1.05 x and +inf; the raw rows are f32 (the data tensor itself, borrowed) and f16 (its .half()).
    Per leg `x<rank>_r<which>_<raw>`: calls/s and the scan stage's kernel time (the library's event pairs), beside the
    estimate-only range search at the same r (legs `est_r...`, rerank off); candidates (the estimate-only totals) and matches per
    query; the raw bytes the exact step requests per call (candidates x dim x element bytes) and per second of the time the scan
    kernel takes beyond the estimate-only kernel at the same r.  Every leg is bounded: windows are cut to --window-s, and a leg that
    has used --leg-limit-s takes no further rounds (its record says how many it took)."""
    rows = {"f32": x_rows, "f16": x_rows.half().contiguous()}
    ebytes = {"f32": 4, "f16": 2}
    bufs = {}

    def configure(raw, r, x):
        if raw is None:
            idx.set_rerank_vectors(None)
        else:
            idx.set_rerank_vectors(device_ptr=rows[raw].data_ptr(), n=a.n, dtype=raw)
        idx.set_range_exact(x)
        idx.set_range_search(r)

    def run(k, calls):
        if k not in bufs:
            bufs[k] = (torch.zeros(a.batch, k, dtype=torch.int64, device=dev), torch.zeros(a.batch, k, dtype=torch.float32, device=dev),
                       torch.zeros(a.batch, dtype=torch.int32, device=dev))
        d_i, d_s, d_c = bufs[k]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            idx.search_batch_device(q.data_ptr(), a.batch, a.dim, k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, d_s, d_c

    kx = max(a.exact_ranks)
    print("index built", file=sys.stderr, flush=True)
    idx.set_rerank_vectors(device_ptr=rows["f32"].data_ptr(), n=a.n, dtype="f32", pool=1024)
    _, d_s, d_c = run(kx, 1)
    idx.set_rerank_pool(0)
    assert int(d_c.min()) == kx, "a query of the sample has fewer results than the largest rank"
    exact_d = d_s.cpu().numpy()
    rec = {"n": a.n, "dim": a.dim, "nlist": a.nlist, "bits": 7, "metric": "L2", "batch": a.batch, "nprobe": a.nprobe, "dataset": "mixture_id32",
           "calls_per_window": a.calls, "window_s": a.window_s, "rounds": a.rounds, "leg_limit_s": a.leg_limit_s, "legs": {}}
    L = []
    inf = float("inf")
    for rank in a.exact_ranks:
        x = float(np.median(exact_d[:, rank - 1]))
        for which, r in (("x", x), ("1.05x", float(np.float32(1.05 * x))), ("inf", inf)):
            est = f"est_r{r:.6g}"
            if est not in rec["legs"]:
                configure(None, r, None)
                cand = run(1, 1)[2].cpu().numpy().astype(np.int64)  # (the totals do not depend on the capacity)
                rec["legs"][est] = {"radius": r if r != inf else "inf", "capacity": max(int(cand.max()), 1), "candidates_total": int(cand.sum()),
                                    "candidates_median": float(np.median(cand)), "candidates_max": int(cand.max())}
                L.append((est, None, r, None, rec["legs"][est]["capacity"]))
            for raw in ("f32", "f16"):
                name = f"x{rank}_r{which}_{raw}"
                configure(raw, r, x)
                tot = run(1, 1)[2].cpu().numpy().astype(np.int64)
                e = rec["legs"][est]
                rec["legs"][name] = {"x": x, "x_rank": rank, "radius": r if r != inf else "inf", "raw": raw, "estimate_only_leg": est, "capacity": max(int(tot.max()), 1),
                                     "matches_total": int(tot.sum()), "matches_median": float(np.median(tot)), "matches_max": int(tot.max()),
                                     "candidates_total": e["candidates_total"], "candidates_median": e["candidates_median"],
                                     "raw_bytes_per_call": e["candidates_total"] * a.dim * ebytes[raw]}
                L.append((name, raw, r, x, rec["legs"][name]["capacity"]))
    times, used = {leg[0]: [] for leg in L}, {leg[0]: 0.0 for leg in L}
    for name, raw, r, x, cap in L:
        print("leg", name, rec["legs"][name], file=sys.stderr, flush=True)
        configure(raw, r, x)
        t0 = time.perf_counter()
        one = min(run(cap, 1)[0] for _ in range(2))  # (the first call sizes the workspace)
        calls = int(max(2, min(a.calls, a.window_s / one)))
        run(cap, calls)  # warm-up window
        rec["legs"][name]["calls"] = calls
        used[name] += time.perf_counter() - t0
    for rnd in range(a.rounds):
        print("round", rnd, file=sys.stderr, flush=True)
        for name, raw, r, x, cap in L:
            if used[name] >= a.leg_limit_s:
                continue
            configure(raw, r, x)
            t0 = time.perf_counter()
            times[name].append(run(cap, rec["legs"][name]["calls"])[0] / rec["legs"][name]["calls"])
            used[name] += time.perf_counter() - t0
    for name, ts in times.items():
        if not ts:
            rec["legs"][name]["rounds_taken"] = 0
            continue
        cps = sorted(1.0 / t for t in ts)
        rec["legs"][name].update({"rounds_taken": len(ts), "calls_per_s_median": round(statistics.median(cps), 3), "calls_per_s_min": round(cps[0], 3),
                                  "calls_per_s_max": round(cps[-1], 3), "queries_per_s_median": round(a.batch * statistics.median(cps)),
                                  "ms_per_call_median": round(1e3 * statistics.median(ts), 4)})
    for name, raw, r, x, cap in L:  # the scan stage's kernel, timed by the library's event pairs: a pass of its own
        configure(raw, r, x)
        idx.set_option("profile_counters", 0)
        idx.profile_begin(stages=("scan",))
        run(cap, max(2, min(rec["legs"][name]["calls"], 5)))
        idx.profile_end()
        s = np.sort(idx.profile_stage_samples("scan"))
        rec["legs"][name].update({"scan_kernel_ms_median": round(float(np.median(s)), 4), "scan_kernel_ms_min": round(float(s[0]), 4),
                                  "scan_kernel_ms_max": round(float(s[-1]), 4), "scan_kernel_samples": int(len(s))})
    for name, raw, r, x, cap in L:
        if raw is None:
            continue
        leg, e = rec["legs"][name], rec["legs"][rec["legs"][name]["estimate_only_leg"]]
        extra_ms = leg["scan_kernel_ms_median"] - e["scan_kernel_ms_median"]
        leg["scan_kernel_ms_over_estimate_only"] = round(extra_ms, 4)
        leg["raw_GB_per_s_of_the_extra_time"] = round(leg["raw_bytes_per_call"] / (extra_ms * 1e-3) / 1e9, 1) if extra_ms > 0 else None
        if "calls_per_s_median" in leg and "calls_per_s_median" in e:
            leg["calls_per_s_over_estimate_only"] = round(leg["calls_per_s_median"] / e["calls_per_s_median"], 4)
    idx.set_range_search(None)
    idx.set_range_exact(None)
    idx.release_stream(st.cuda_stream)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ranks", nargs="+", type=int, default=[10, 100, 1000], help="the radius is the median distance at these ranks")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--window-s", type=float, default=2.0, help="a window is cut to about this long (at least two calls)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", required=True)
    ap.add_argument("--exact", action="store_true", help="the legs of the exact range search (DESIGN.md section 33) instead")
    ap.add_argument("--exact-ranks", nargs="+", type=int, default=[10, 100], help="x is the median exact distance at these ranks")
    ap.add_argument("--leg-limit-s", type=float, default=40.0, help="--exact: a leg stops taking rounds once it has used this long")
    a = ap.parse_args()
    import torch
    import bench
    import rabitq_rs_amd as rq
    dev = torch.device("cuda", 0)
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
    st = torch.cuda.Stream(dev)
    bufs = {}

    def run(radius, k, calls):
        """`calls` calls at top_k / capacity k: the range search with a radius, the top-k search with None"""
        if k not in bufs:
            bufs[k] = (torch.zeros(a.batch, k, dtype=torch.int64, device=dev), torch.zeros(a.batch, k, dtype=torch.float32, device=dev),
                       torch.zeros(a.batch, dtype=torch.int32, device=dev))
        d_i, d_s, d_c = bufs[k]
        idx.set_range_search(radius)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            idx.search_batch_device(q.data_ptr(), a.batch, a.dim, k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        idx.set_range_search(None)
        return dt, d_s, d_c

    if a.exact:
        exact_legs(a, torch, dev, idx, x, q, st)
        return
    kmax = max(a.ranks)
    _, d_s, d_c = run(None, kmax, 1)
    assert int(d_c.min()) == kmax, "a query of the sample has fewer results than the largest rank"
    dist = d_s.cpu().numpy()
    rec = {"n": a.n, "dim": a.dim, "nlist": a.nlist, "bits": 7, "metric": "L2", "batch": a.batch, "nprobe": a.nprobe, "dataset": "mixture_id32",
           "calls_per_window": a.calls, "window_s": a.window_s, "rounds": a.rounds, "legs": {}}
    L = []
    for rank in a.ranks:
        r = float(np.median(dist[:, rank - 1]))
        _, _, d_c = run(r, 1, 1)  # the totals do not depend on the capacity
        tot = d_c.cpu().numpy().astype(np.int64)
        cap = max(int(tot.max()), 1)
        # (`_topk_at_rank`: the top-k search at top_k := the rank itself — what it costs to get the median query's set, truncated for
        # the others)
        for name, radius, k in ((f"rank{rank}_range", r, cap), (f"rank{rank}_topk", None, cap), (f"rank{rank}_topk_at_rank", None, rank)):
            one = min(run(radius, k, 1)[0] for _ in range(2))  # (the first call sizes the workspace)
            calls = int(max(2, min(a.calls, a.window_s / one)))
            run(radius, k, calls)  # warm-up window
            rec["legs"][name] = {"radius": r, "rank": rank, "capacity": k, "matches_total": int(tot.sum()), "matches_median": float(np.median(tot)),
                                 "matches_max": int(tot.max()), "calls": calls}
            L.append((name, radius, k, calls))
    times = {leg[0]: [] for leg in L}
    for _ in range(a.rounds):
        for name, radius, cap, calls in L:
            times[name].append(run(radius, cap, calls)[0] / calls)
    for name, ts in times.items():
        qps = sorted(a.batch / t for t in ts)
        rec["legs"][name].update({"queries_per_s_median": round(statistics.median(qps)), "queries_per_s_min": round(qps[0]),
                                  "queries_per_s_max": round(qps[-1]), "ms_per_call_median": round(1e3 * statistics.median(ts), 4)})
    for name, radius, cap, calls in L:  # the scan stage's kernel, timed by the library's event pairs: a pass of its own
        idx.set_option("profile_counters", 0)
        idx.profile_begin(stages=("scan",))
        run(radius, cap, max(2, min(calls, 7)))
        idx.profile_end()
        s = np.sort(idx.profile_stage_samples("scan"))
        rec["legs"][name].update({"scan_kernel_ms_median": round(float(np.median(s)), 4), "scan_kernel_ms_min": round(float(s[0]), 4),
                                  "scan_kernel_ms_max": round(float(s[-1]), 4), "scan_kernel_samples": int(len(s))})
    idx.release_stream(st.cuda_stream)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
