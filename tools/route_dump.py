"""Which kernels a search call runs, for a grid of call shapes and every option that forces a route: stage_resources() of three
small indexes as JSON lines (nothing is launched).  Two builds that route alike print the same lines:

  python tools/route_dump.py OUT.jsonl                 # this tree's library
  RBQ_LIB_PATH=.../librbq.so python tools/route_dump.py OTHER.jsonl
  diff OUT.jsonl OTHER.jsonl

One line per (index, option): {"call": "<index>/<option>", "<nq>": {stage: ...}, ...} holds the 15 (top_k, nprobe) calls of every
nq, per stage [workgroups, threads, vgprs, lds_bytes, scratch_bytes], the rank stage with its operand format.  Written without
repetition, nothing left out: a stage that is the same for the 15 calls stands once; else {"k=<top_k>,<top_k>..": ...} groups the
top_k that agree, and below that {"p=<nprobe>": ...} where nprobe matters.  Under a forced option only what differs from the
default line of the same index is written: an absent stage, or nq, equals the default's.  tests/test_gpu_search_plan.py replays the
first two indexes against tests/golden/search_routes.jsonl (--golden FILE writes that file: workgroups, threads and operands only
- registers and LDS belong to the kernels)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (n, dim, n_lists, total_bits, rotator): 1-bit; 7-bit FHT-Kac with many lists; the matrix rotator
INDEXES = [(8192, 64, 64, 1, 1), (8192, 256, 4096, 7, 1), (3000, 64, 24, 7, 0)]
NQ = (1, 4, 5, 64, 65, 128, 512, 513, 768, 1024)
TOP_K = (1, 10, 100, 256, 300)
NPROBE = (1, 16, 0)  # 0: every list
# option, forced value, default
FORCED = [("rank_tile", 64, 0), ("rank_tile", 128, 0), ("rank_tile", 256, 0), ("rank_f16", 0, -1), ("rank_f16", 1, -1),
          ("rank_ksplit", 0, 1), ("rank_ksplit", 3, 1), ("rank_ksplit", 8, 1), ("exact_rank", 1, 0), ("f32_rank", 1, 0), ("wg_prep", 1, 0),
          ("rank_planar", 1, 0), ("latency_path", 0, 1), ("scan_wave", 0, -1), ("scan_wave", 1, -1), ("block_bound", 0, 1)]
STAGES = ("prep", "rank", "select", "scan")


def build(i):
    """Index i of INDEXES: seeded Gaussian data around seeded centroids, vector v in list v % n_lists (no k-means: the routes read
    the geometry, not the clustering)."""
    import rabitq_rs_amd as rq
    n, dim, nlist, bits, rotator = INDEXES[i]
    rng = np.random.default_rng(7100 + i)
    cent = rng.standard_normal((nlist, dim)).astype(np.float32)
    assign = (np.arange(n) % nlist).astype(np.uint32)
    data = cent[assign] + 0.25 * rng.standard_normal((n, dim)).astype(np.float32)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, 0, rotator, 7200 + i, True)
    return rq.IvfRabitqIndex.from_built(built)


def routes(idx, i):
    """("<index>/<option>", {nq: {(top_k, nprobe): stage_resources}}) over the grid: the default options, then every forced one in turn"""
    nlist = INDEXES[i][2]
    for name, value, default in [(None, 0, 0)] + FORCED:
        if name:
            idx.set_option(name, value)
        yield ("%d/%s" % (i, "%s=%d" % (name, value) if name else "default"),
               {nq: {(k, p or nlist): idx.stage_resources(nq, k, p or nlist) for k in TOP_K for p in NPROBE} for nq in NQ})
        if name:
            idx.set_option(name, default)


def full_row(res):
    return {s: [res[s][f] for f in ("workgroups", "threads", "vgprs", "lds_bytes", "scratch_bytes")] + ([res[s]["operands"]] if s == "rank" else [])
            for s in STAGES}


def golden_row(res):
    """what the golden keeps of one call: workgroups and threads per stage, the rank stage's operands"""
    return {s: [res[s]["workgroups"], res[s]["threads"]] + ([res[s]["operands"]] if s == "rank" else []) for s in STAGES}


def fold(cells):
    """{(top_k, nprobe): value} as written: the top_k with the same nprobe -> value map share an entry, a map of one value is that value"""
    by_k, groups = {}, []
    for (k, p), v in cells.items():
        by_k.setdefault(k, {})[p] = v
    for k, m in by_k.items():
        for g in groups:
            if g[1] == m:
                g[0].append(k)
                break
        else:
            groups.append([[k], m])

    def inner(m):
        vs = list(m.values())
        return vs[0] if all(v == vs[0] for v in vs) else {"p=%d" % p: v for p, v in m.items()}
    return inner(groups[0][1]) if len(groups) == 1 else {"k=" + ",".join(map(str, ks)): inner(m) for ks, m in groups}


class Writer:
    """the lines of one output: calls reduced by `row` (full_row or golden_row), folded, forced options against the default's line"""

    def __init__(self, row):
        self.row, self.default, self.lines = row, {}, []

    def add(self, key, per_nq):
        index, option = key.split("/")
        out = {"call": key}
        for nq, calls in per_nq.items():
            rows = {kp: self.row(res) for kp, res in calls.items()}
            folded = {s: fold({kp: r[s] for kp, r in rows.items()}) for s in STAGES}
            if option == "default":
                self.default[index, nq] = folded
            else:
                folded = {s: f for s, f in folded.items() if f != self.default[index, nq][s]}
            if folded:
                out[str(nq)] = folded
        self.lines.append(json.dumps(out, separators=(",", ":")))
        return self.lines[-1]


def main(argv):
    golden = None
    if len(argv) >= 2 and argv[0] == "--golden":
        golden, argv = argv[1], argv[2:]
    if len(argv) != 1:
        sys.exit(__doc__)
    full, kept = Writer(full_row), Writer(golden_row)
    for i in range(len(INDEXES)):
        idx = build(i)
        for key, per_nq in routes(idx, i):
            full.add(key, per_nq)
            if i < 2:
                kept.add(key, per_nq)
        idx.close()
    for path, w in ((argv[0], full), (golden, kept)):
        if path:
            with open(path, "w") as f:
                f.write("".join(l + "\n" for l in w.lines))
    print("route_dump: %d indexes, %d calls each -> %s" % (len(INDEXES), (1 + len(FORCED)) * len(NQ) * len(TOP_K) * len(NPROBE), argv[0]))


if __name__ == "__main__":
    main(sys.argv[1:])
