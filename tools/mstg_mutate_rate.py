"""Cost of changing a device-resident MSTG index with rbq_mstg_append / rbq_mstg_remove_ids against the only thing the library
offered before them: rbq_mstg_build_device over every row the index then holds.

Set-up: a Gaussian mixture in --intrinsic dimensions embedded in 960 (tools/mstg_build_rate.py's), 1 M + 100 k rows resident
on the GPU; the first 1 M are clustered with hierarchical_cluster at the crate's default max_posting_size (5000) and built into
a 7-bit index with the crate's default closure epsilon (0.15) and max_replicas (8).  Then
  the 100 k further rows are appended                          (append_s)      against a build over all 1.1 M rows (rebuild_all_s)
  1 % / 10 % of the ids, drawn at random, are removed          (remove_*_s)    against a build over the kept rows  (rebuild_kept_*_s)
Wall seconds of ONE call after a warm-up call of the same kind, host overheads included; the rebuilds run in the same session
(their warm-up is the base build).  There is no threshold.  Prints one JSON line; --out writes it to a file
(profiles/mstg_mutate_rate.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dataset(torch, n, dim, intrinsic, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    means = torch.randn((64, intrinsic), generator=g, device="cuda")
    proj = torch.randn((intrinsic, dim), generator=g, device="cuda") / float(np.sqrt(intrinsic))
    x = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        low = means[torch.randint(0, 64, (m,), generator=g, device="cuda")] + 0.35 * torch.randn((m, intrinsic), generator=g, device="cuda")
        x[r0:r0 + m] = low @ proj + 0.02 * torch.randn((m, dim), generator=g, device="cuda")
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--add", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--max-posting-size", type=int, default=5000)
    ap.add_argument("--epsilon", type=float, default=0.15)
    ap.add_argument("--max-replicas", type=int, default=8)
    ap.add_argument("--intrinsic", type=int, default=8)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run says nothing about these times")
    import rabitq_rs_amd as rq
    from rabitq_rs_amd import mstg
    eps, m = a.epsilon, a.max_replicas
    x = dataset(torch, a.n + a.add, a.dim, a.intrinsic, a.seed)
    torch.cuda.synchronize()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0

    (cent, _off, _mem, _st), t_cluster = wall(lambda: mstg.hierarchical_cluster(x[:a.n], a.max_posting_size))

    def build(rows):
        return rq.build_postings_on_device(rows, cent, a.bits, 0, eps, m, faster_config=True)

    base, t_base = wall(lambda: build(x[:a.n]))
    base.id_bound()
    rec = {"tool": "mstg_mutate_rate", "n": a.n, "add": a.add, "dim": a.dim, "bits": a.bits, "max_posting_size": a.max_posting_size,
           "epsilon": eps, "max_replicas": m, "intrinsic": a.intrinsic, "lists": int(len(cent)), "cluster_s": round(t_cluster, 4),
           "base_build_s": round(t_base, 4), "base_slots": len(base)}

    new = x[a.n:]
    warm = mstg.append_postings(base, new, a.n, eps, m)
    warm.close()
    grown, t_append = wall(lambda: mstg.append_postings(base, new, a.n, eps, m))
    rec["grown_slots"] = len(grown)
    grown.close()
    full, t_all = wall(lambda: build(x))
    assert len(full) == rec["grown_slots"]
    full.close()
    rec.update({"append_s": round(t_append, 4), "rebuild_all_s": round(t_all, 4), "rebuild_all_over_append": round(t_all / t_append, 2)})

    rng = np.random.default_rng(a.seed)
    for pct in (1, 10):
        gone = np.sort(rng.choice(a.n, a.n * pct // 100, replace=False))
        d_gone = torch.from_numpy(gone).cuda()
        warm, _ = mstg.remove_postings(base, d_gone)
        warm.close()
        (shrunk, removed), t_remove = wall(lambda: mstg.remove_postings(base, d_gone))
        keep = torch.ones(a.n, dtype=torch.bool, device="cuda")
        keep[d_gone] = False
        kept_rows = x[:a.n][keep].contiguous()  # (not timed: the rebuild is given its rows)
        rebuilt, t_kept = wall(lambda: build(kept_rows))
        assert len(rebuilt) == len(shrunk) == len(base) - removed
        rec.update({f"remove_{pct}pct_s": round(t_remove, 4), f"remove_{pct}pct_slots": int(removed),
                    f"rebuild_kept_{pct}pct_s": round(t_kept, 4), f"rebuild_kept_over_remove_{pct}pct": round(t_kept / t_remove, 2)})
        shrunk.close()
        rebuilt.close()
        del kept_rows
    base.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
