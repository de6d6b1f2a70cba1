"""Time of the refined MSTG search (rbq_mstg_search_refined_batch*) next to the plain one (rbq_mstg_search_batch*) on one handle:
N = 1 M vectors of dim 960, 7 bits, L2, batches of 1024 queries, the `balanced` preset (ef_search 150, pruning_epsilon 0.6),
about 1000 lists.  One pool per process (--pool 100 and 1000 are the two recorded shapes), each under a time limit of its own,
and nothing is started after a failure:

  timeout -k 10 900 python tools/mstg_refine_rate.py --pool 100  --out profiles/mstg_refine_rate_100.json &&
  timeout -k 10 900 python tools/mstg_refine_rate.py --pool 1000 --out profiles/mstg_refine_rate_1000.json

Every leg is the wall time of the whole call, one warm-up run and then the median of --repeats runs; the device legs are timed
between stream synchronisations.  The record also holds how many of the plain call's top_k slots carry an id a second time and
the mean number of ids the refined call returns."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, required=True)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    from mstg_build_rate import dataset
    from mstg_search_rate import timed
    p = rq.MstgSearchParams.balanced()
    k = a.lists * a.n // 1000000 or 1
    x = dataset(a.n, a.dim, 32, 1)
    cent = np.ascontiguousarray(x[:: a.n // k][:k])
    rng = np.random.default_rng(2)
    q = (x[rng.integers(0, a.n, a.batch)] + 0.02 * rng.standard_normal((a.batch, a.dim))).astype(np.float32)
    idx = rq.build_postings_on_device(x, cent, 7, 0, faster_config=True)
    args = (a.top_k, p.ef_search, p.pruning_epsilon)
    rec = {"n": a.n, "dim": a.dim, "n_lists": k, "batch": a.batch, "top_k": a.top_k, "ef_search": p.ef_search,
           "pruning_epsilon": p.pruning_epsilon, "refine_pool": a.pool, "stored_vectors": len(idx)}
    ids, _, cnt = rq.mstg_search(idx, q, *args)
    rec["plain_repeated_slots_per_query"] = round(float(np.mean([int(cnt[i]) - len(set(ids[i, :int(cnt[i])].tolist())) for i in range(len(q))])), 3)
    rids, _, rcnt = rq.mstg_search(idx, q, *args, refine_pool=a.pool)
    rec["refined_rows_unique"] = bool(all(len(set(rids[i, :int(rcnt[i])].tolist())) == int(rcnt[i]) for i in range(len(q))))
    rec["refined_mean_count"] = round(float(rcnt.mean()), 3)
    rec["plain_host"] = timed(lambda: rq.mstg_search(idx, q, *args), a.repeats)
    rec["refined_host"] = timed(lambda: rq.mstg_search(idx, q, *args, refine_pool=a.pool), a.repeats)
    tq = torch.from_numpy(q).cuda()

    def dev(pool):
        rq.mstg_search(idx, tq, *args, refine_pool=pool)
        torch.cuda.synchronize()
    rec["plain_device"] = timed(lambda: dev(None), a.repeats)
    rec["refined_device"] = timed(lambda: dev(a.pool), a.repeats)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
