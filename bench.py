#!/usr/bin/env python3
"""bench.py — queries/sec of the IVF+RaBitQ candidate-scan path on MI355X.

A "step" is one pass of the hot path (rotate -> LUT -> centroid ranking -> code scan -> prune -> ex-refine
-> top-k) over one batch of synthetic queries, inputs already resident in HBM.  Workload at N=1 = the
configuration BASELINE.json's metric is quoted on: GIST-1M-shaped synthetic fvecs (N=1M, d=960),
nlist=4096, 7-bit codes, FhtKacRotator, L2, nprobe=128, top_k=10, batch=1024.

Every step searches a DIFFERENT query batch: --nbatches (default 32) distinct batches are drawn per rank and the
steps walk through them round-robin, so no step finds its predecessor's code blocks or centroid rows in the cache
(a serving workload never sees the same batch twice).

Multi-GPU (--gpus N): index replicated per rank, each rank searches its own batches (weak scaling, no data-path
collective), then ONE RCCL all_gather of the [batch][top_k] (id, score) blocks per bucket of batches — the only exchange
the path has.  `python bench.py --gpus N` starts its own N ranks (a child `torch.distributed.run`, before
this process touches the GPU); under torch.distributed.run it runs as a rank.  --in-library: ONE process, ONE handle with
N replicas, host buffers through rbq_search_batch (the reference's batch_search binding).

The timed region is exactly K = --steps steps (barrier + synchronize on both sides, max over ranks); `ms_per_step` is its
duration / K.  With --min-seconds S > 0 the region is repeated until S seconds have been measured and `value` is the median
region (`timed_regions`, `region_ms`).

--dump-outputs DIR writes what the timed path returned in its last timed step (ids, scores, counts of that batch, as float64 /
float32 .npy files) and the batch's queries.  Inputs are seeded and the harness k-means is deterministic, so two runs with the
same arguments search the same index with the same queries and their dumps can be compared file by file.

A plain run (no --full) does what the headline figure needs and nothing else: it builds the index and the exact ground truth,
warms up, times the K steps, writes --dump-outputs, measures the recall that `metric` states (every batch once more on one
stream, against the ground truth) and prints the line; every object below `value / ms_per_step` is then null.  --full adds the
supplementary legs (each takes GPU or CPU runs of its own): the counter pass behind `pruned`, `roofline`, the per-stage pass and
`regime`, the GPU encoder comparison, `host_call` / `pcie_inclusive`, `latency`, `self_check`, `datasets`, `sensitivity` and
`cpu_baseline`; --no-cpu, --no-extras, --no-latency, --ab and --no-wave-roofline trim a --full run and mean nothing without it.
The timed region, its inputs and the dumped arrays are the same with and without --full.  (--in-library is a mode of its own:
one measurement with its own checks, the same with and without --full.)

Prints one JSON line (rank 0).  What the objects mean:
  value / ms_per_step   whole path, queries and results resident in HBM, batches pipelined over --streams HIP streams
  roofline              k_scan with the block-level bound switched OFF (every probed block streamed, results
                        identical): algorithmic bytes (sum_q sum_{c in probe(q)} n_c*(D/8+12)) / HIP-event
                        launch time — a true HBM-roofline position (<= 1)
  pruned                the product configuration (bound ON) of the timed region: bytes the kernel actually requested,
                        counted inside the kernel in the same launches, block skip fraction, frac = requested/time/peak
  host_call             THE CALL THE REFERENCE BINDS: one rbq_search_batch call per step from one caller thread (host buffers in and
                        out, distinct batches), median call — what a Rust / Python caller of the drop-in sees; `value` stays the
                        device-resident rate (bench contract: inputs in HBM when the timed region starts)
  pcie_inclusive        the same entry point with 1 and 4 caller threads, pageable and page-locked buffers, 1 and 4 batches per call
  regime                what bounds the timed (pruned) configuration: every stage's duration under overlap, resident waves x time per
                        query against the chip's wave slots
  sensitivity           lists scanned / queries/s / recall against the intrinsic dimension of the data (16 ... 128, isotropic)
  datasets              the low-intrinsic-dimension mixture (headline) and SURVEY 8d's isotropic mixture, each with recall,
                        rate and skip fraction
  cpu_baseline          the oracle (C restatement of the reference's AVX2/AVX-512 FastScan path) on the host cores: median
                        of 3 passes on the fastest thread count of a short sweep, plus the single-thread figure (how the
                        reference times itself)
  latency               p50 / p99 of ONE rbq_search_batch call at nq in {1, 4, 8, 64, 256} (page-locked buffers); nq 1 and 64 also through the batch kernels
  self_check            256 queries again with every shortcut off (exact all-pairs ranking, BinaryHeap emulation, no block
                        bound): identical bits — the check that also covers indexes no CPU oracle run can (cfg5)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The HIP runtime multiplexes a process's streams over its default number of hardware queues; the benchmark leaves that
# count alone (raising it is a machine-wide setting on shared machines, and more queues than the card's slots has hung one).

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8 TB/s
# HBM bytes per bound-off k_scan launch of the HEADLINE configuration from the committed PMC pass of this build (FETCH_SIZE x 2 on
# gfx950, its own rocprofv3 run: profiles/r5/summary_headline.md).  PMC counters cannot be read inside a normal bench run, so
# roofline.traffic carries this figure (and says where it comes from); tools/profile_round.sh regenerates it.
PMC_TRAFFIC = {"bytes": None, "source": None}
try:
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r5", "pmc_traffic.json")) as _f:
        PMC_TRAFFIC = json.load(_f)
except Exception:  # noqa: BLE001
    pass
HEADLINE = dict(n=1_000_000, dim=960, nlist=4096, nprobe=128, bits=7, metric=0, batch=1024, top_k=10)
# BASELINE.json `configs` by name; cfg3 = the headline; the reference's own benchmark setting is top_k = 100
# (examples/recall_qps_sweep.rs:111,120,225-237)
PRESETS = {
    "cfg2": dict(n=1_000_000, dim=128, nlist=1024, nprobe=64, bits=7, metric=0, batch=1024, top_k=10),
    "cfg3": dict(HEADLINE),
    "cfg3_b4096": dict(HEADLINE, batch=4096, nbatches=8),
    "cfg4": dict(n=1_000_000, dim=960, nlist=4096, nprobe=256, bits=3, metric=1, batch=1024, top_k=10),
    "top100": dict(HEADLINE, top_k=100),
    "cfg5": dict(n=100_000_000, dim=768, nlist=65536, nprobe=512, bits=7, metric=0, batch=16384, top_k=10, nbatches=2,
                 stream_build=2_000_000, steps=8, warmup=2, streams=4),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--n", type=int, default=HEADLINE["n"])
    ap.add_argument("--dim", type=int, default=HEADLINE["dim"])
    ap.add_argument("--nlist", type=int, default=HEADLINE["nlist"])
    ap.add_argument("--nprobe", type=int, default=HEADLINE["nprobe"])
    ap.add_argument("--bits", type=int, default=HEADLINE["bits"])
    ap.add_argument("--metric", type=int, default=HEADLINE["metric"])
    ap.add_argument("--batch", type=int, default=HEADLINE["batch"])
    ap.add_argument("--top-k", type=int, default=HEADLINE["top_k"])
    ap.add_argument("--nbatches", type=int, default=32, help="distinct query batches the steps rotate through")
    ap.add_argument("--full", action="store_true",
                    help="also run the supplementary legs (counter pass, roofline, per-stage pass, GPU encoder comparison, host entry, "
                         "latency, self check, other data sets, CPU baseline); without it only what the headline figure needs runs")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU-baseline sample duration")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--ab", action="store_true", help="kernel A/B runs: only the per-stage pass of the supplementary legs")
    ap.add_argument("--no-extras", action="store_true", help="skip the supplementary legs (second data set, host API, per-stage pass)")
    ap.add_argument("--dataset", default="mixture_id32", choices=["mixture_id16", "mixture_id32", "mixture_id64", "mixture_id128", "isotropic"],
                    help="headline data: low-intrinsic-dimension mixture (default) or SURVEY 8d's isotropic mixture")
    ap.add_argument("--device-build", action="store_true",
                    help="build the index with the GPU-side encoder only (large n: no CPU build, no oracle check)")
    ap.add_argument("--stream-build", type=int, default=0, metavar="CHUNK",
                    help="build with the streamed encoder, CHUNK vectors at a time, regenerating the data per chunk "
                         "(indexes whose raw vectors exceed HBM: cfg5)")
    ap.add_argument("--kmeans-iters", type=int, default=6)
    ap.add_argument("--option", action="append", default=[], help="rbq_debug_set_option name=value (diagnostic A/B runs)")
    ap.add_argument("--streams", type=int, default=12, help="HIP streams the batches are issued on, round-robin (tools/streams_sweep.py)")
    ap.add_argument("--config", default=None, choices=sorted(PRESETS),
                    help="a BASELINE.json configuration by name (sets n/dim/nlist/nprobe/bits/metric/batch/top-k; explicit flags win)")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="the K-step timed region is repeated (each repeat bracketed by barrier + synchronize) until this much "
                         "time has been measured; value = median region (default 0: one region, exactly --steps timed steps)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the outputs of the last timed step (what a caller of the timed path receives) as DIR/<name>.npy")
    ap.add_argument("--in-library", action="store_true",
                    help="ONE process, ONE handle with --gpus replicas, host buffers through rbq_search_batch (the reference's "
                         "batch_search binding, src/ivf.rs:1743-1752) instead of one process per GPU")
    ap.add_argument("--caller-threads", type=int, default=1, help="--in-library: host threads calling rbq_search_batch concurrently")
    ap.add_argument("--no-latency", action="store_true", help="skip the small-batch latency leg")
    ap.add_argument("--no-wave-roofline", action="store_true",
                    help="skip the roofline leg's second half (the bound-off configuration through k_scanw): counter passes of "
                         "tools/profile_round.sh, whose per-kernel medians should not be dominated by eager-selection launches")
    argv = json.loads(os.environ["RBQ_BENCH_ARGV"]) if (os.environ.get("RBQ_BENCH_ARGV") and len(sys.argv) == 1) else sys.argv[1:]
    a = ap.parse_args(argv)
    if a.config:
        given = {w.split("=")[0] for w in argv if w.startswith("--")}
        for k, v in PRESETS[a.config].items():
            if "--" + k.replace("_", "-") not in given:
                setattr(a, k, v)
    return a


INTRINSIC_DIM = 32  # GIST-like: neighbours live on a low-dimensional manifold, not an isotropic ball


class Mixture:
    """Synthetic GIST-1M-shaped fvecs: Gaussian mixture with nlist/4 component means ~ N(0, I_d).
    kind == "mixture_id32": intrinsic dimension 32, x = mean_k + 0.35 * z A / sqrt(32) + 0.1 * eps  (z in R^32)
    kind == "isotropic":    SURVEY.md 8d's recipe, x = mean_k + 0.35 * N(0, I_d).  In d=960 that makes the 10 nearest
                            neighbours equidistant to within 3.6 % (d10/d1 = 1.036) and caps recall@10 of the reference's
                            own estimator near 0.93 for ANY nprobe — reported, never the headline."""

    def __init__(self, torch, dev, dim, nlist, kind, normalize):
        self.torch, self.dev, self.dim, self.kind, self.normalize = torch, dev, dim, kind, normalize
        self.kgen = max(nlist // 4, 1)
        # "mixture_idN": intrinsic dimension N (the headline is N = 32; the sensitivity leg sweeps it)
        self.idim = int(kind[len("mixture_id"):]) if kind.startswith("mixture_id") else INTRINSIC_DIM
        gm = torch.Generator(device=dev)
        gm.manual_seed(20260101)
        self.means = torch.randn(self.kgen, dim, generator=gm, device=dev)
        self.A = torch.randn(self.idim, dim, generator=gm, device=dev) / (self.idim ** 0.5)

    def draw(self, n, seed):
        torch, dev = self.torch, self.dev
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        comp = torch.randint(0, self.kgen, (n,), generator=g, device=dev)
        x = torch.empty(n, self.dim, device=dev)
        for s in range(0, n, 131072):
            e = min(n, s + 131072)
            if self.kind == "isotropic":
                x[s:e] = self.means[comp[s:e]] + 0.35 * torch.randn(e - s, self.dim, generator=g, device=dev)
            else:
                z = torch.randn(e - s, self.idim, generator=g, device=dev)
                x[s:e] = self.means[comp[s:e]] + 0.35 * (z @ self.A) + 0.1 * torch.randn(e - s, self.dim, generator=g, device=dev)
        if self.normalize:
            x /= x.norm(dim=1, keepdim=True)
        return x


def kmeans_gpu(torch, x, k, iters, seed):
    """Harness k-means on the GPU (the reference accepts external clusters: train_with_clusters)."""
    n = x.shape[0]
    g = torch.Generator(device=x.device)
    g.manual_seed(seed)
    cent = x[torch.randperm(n, generator=g, device=x.device)[:k]].clone()
    assign = torch.empty(n, dtype=torch.int64, device=x.device)
    for it in range(iters + 1):
        assign = assign_gpu(torch, x, cent, assign)
        if it == iters:
            break
        # index_put_ with accumulate sorts the indices and adds in a fixed order (index_add_ uses atomics: the centroids, and
        # with them a few list assignments, would change from run to run)
        sums = torch.zeros_like(cent).index_put_((assign,), x, accumulate=True)
        cnt = torch.bincount(assign, minlength=k).clamp(min=1).unsqueeze(1)
        newc = sums / cnt
        empty = (torch.bincount(assign, minlength=k) == 0)
        if empty.any():
            newc[empty] = x[torch.randint(0, n, (int(empty.sum()),), generator=g, device=x.device)]
        cent = newc
    return cent, assign


def assign_gpu(torch, x, cent, out=None):
    n = x.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=x.device)
    cn = (cent * cent).sum(1)
    step = max(1024, min(65536, (1 << 31) // max(cent.shape[0], 1)))
    for s in range(0, n, step):
        e = min(n, s + step)
        out[s:e] = (cn[None, :] - 2.0 * (x[s:e] @ cent.T)).argmin(1)
    return out


def exact_topk_update(torch, best, xs, base, q, k, metric):
    """merge the exact top-k of queries q against the chunk xs (ids base..) into best = (values, ids)"""
    for qs in range(0, q.shape[0], 4096):
        qq = q[qs:qs + 4096]
        for s in range(0, xs.shape[0], 262144):
            xc = xs[s:s + 262144]
            if metric == 0:
                d = (qq * qq).sum(1, keepdim=True) - 2.0 * (qq @ xc.T) + (xc * xc).sum(1)[None, :]
                v, i = d.topk(min(k, xc.shape[0]), dim=1, largest=False)
            else:
                v, i = (qq @ xc.T).topk(min(k, xc.shape[0]), dim=1, largest=True)
            i = i + (base + s)
            bv, bi = best[0][qs:qs + 4096], best[1][qs:qs + 4096]
            cv, ci = torch.cat([bv, v], 1), torch.cat([bi, i], 1)
            sv, si = cv.topk(k, dim=1, largest=(metric != 0))
            best[0][qs:qs + 4096] = sv
            best[1][qs:qs + 4096] = torch.gather(ci, 1, si)


def exact_topk(torch, x, q, k, metric):
    fill = float("inf") if metric == 0 else float("-inf")
    best = [torch.full((q.shape[0], k), fill, device=q.device), torch.full((q.shape[0], k), -1, dtype=torch.int64, device=q.device)]
    exact_topk_update(torch, best, x, 0, q, k, metric)
    return best[1]


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, ids, scores, counts, queries):
    """The last timed step's results, as a caller of the timed path receives them: ids [nq][top_k] (uint64, written as float64:
    exact below 2^53, the empty-slot sentinel 2^64 - 1 rounds to 2^64), scores [nq][top_k] float32, counts [nq] (float64) and
    the queries of that step [nq][dim] float32.  Above DUMP_LIMIT_BYTES a fixed, seeded sample of the queries' rows is written
    (`rows` holds their indices)."""
    nq = ids.shape[0]
    row_bytes = ids.shape[1] * 12 + 16 + queries.shape[1] * 4  # ids f64 + scores f32, counts f64, rows f64, queries f32
    budget = DUMP_LIMIT_BYTES - 4096  # (.npy headers)
    rows = np.arange(nq)
    if nq * row_bytes > budget:
        rows = np.sort(np.random.default_rng(20260106).choice(nq, budget // row_bytes, replace=False))
    os.makedirs(d, exist_ok=True)
    arrays = {"ids": ids[rows].astype(np.float64), "scores": scores[rows].astype(np.float32), "counts": counts[rows].astype(np.float64),
              "queries": queries[rows].astype(np.float32), "rows": rows.astype(np.float64)}
    for name, v in arrays.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(v))


def recall_of(ids, gt, k):
    """mean |returned ∩ exact top-k| / k; ids, gt: [nq][k] integer arrays"""
    hit = (ids[:, :, None].astype(np.int64) == gt[:, None, :].astype(np.int64)).any(axis=2).sum(axis=1)
    return float(hit.mean() / k)


class TopkExchange:
    """The path's only exchange: every rank's [batch][top_k] ids (u64 bit patterns) and scores live in ONE
    packed buffer per result slot, `bucket` consecutive slots are contiguous, and the final top-k exchange is a single
    all_gather per bucket (bucket = 1: per batch).  Used by the timed loop on HBM buffers over RCCL and by
    tests/test_dist_gloo.py on CPU buffers over gloo."""

    def __init__(self, torch, dev, batch, top_k, nslots, world, gather, single_rank_group=False, bucket=1):
        self.torch, self.batch, self.top_k, self.world, self.bucket = torch, batch, top_k, world, bucket
        nres = batch * top_k
        self.nb = nres * 12
        self.buf = torch.empty(nslots * self.nb, dtype=torch.uint8, device=dev)
        self.pack = [self.buf[i * self.nb:(i + 1) * self.nb] for i in range(nslots)]
        self.ids = [p[:nres * 8].view(torch.int64).view(batch, top_k) for p in self.pack]
        self.scores = [p[nres * 8:].view(torch.float32).view(batch, top_k) for p in self.pack]
        self.counts = [torch.empty(batch, dtype=torch.int32, device=dev) for _ in range(nslots)]
        # gather targets: one set per bucket, so overlapping buckets never share a buffer
        self.gathered = ([[torch.empty(bucket * self.nb, dtype=torch.uint8, device=dev) for _ in range(world)]
                          for _ in range(nslots // bucket)] if (gather and (world > 1 or single_rank_group)) else None)

    def gather(self, dist, b):
        """all_gather of bucket b's packed results, enqueued on the current stream"""
        if self.gathered is not None:
            dist.all_gather(self.gathered[b], self.buf[b * self.bucket * self.nb:(b + 1) * self.bucket * self.nb])

    def unpack(self, slot):
        """(ids [world*batch][top_k] int64, scores) of slot `slot` after its bucket's gather, rank order = query-shard order"""
        nres = self.batch * self.top_k
        off = (slot % self.bucket) * self.nb
        packs = [g[off:off + self.nb] for g in self.gathered[slot // self.bucket]] if self.gathered is not None else [self.pack[slot]]
        ids = self.torch.cat([p[:nres * 8].view(self.torch.int64).view(self.batch, self.top_k) for p in packs])
        sc = self.torch.cat([p[nres * 8:].view(self.torch.float32).view(self.batch, self.top_k) for p in packs])
        return ids, sc


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def traffic_of(c, D, Dc, ex_bits, launches):
    """bytes k_scan requested per launch, from its own counters (rbq_profile_counters)"""
    cpu_u = 128 // ex_bits if ex_bits else 1
    exd = (((D // 16 + cpu_u - 1) // cpu_u) * 256) if ex_bits else 0
    qlen = max(D, (exd // 256) * cpu_u * 16) if ex_bits else D
    b = {"sign_codes": c["code_blocks"] * 4 * Dc, "factor_rows": c["meta_blocks"] * 384, "block_stream": c["stream_entries"] * 16,
         "ex_codes": c["ex_evals"] * (exd + 8), "lut_and_query": c["queries"] * (4 * Dc + 4 * qlen)}
    tot = sum(b.values())
    L = max(launches, 1)
    return tot / L, {k: v / L for k, v in b.items()}


def self_launch(a):
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the N ranks as a CHILD process and relay its
    JSON line and exit code.  Nothing in this (parent) process has touched the GPU: torch.cuda and librbq are imported
    further down, never here, and the child is a new process, not an exec of one that initialised HIP."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # the ranks read their arguments from the environment: torch.distributed.run's own parser would try to match bench
    # flags such as --n against its options (ambiguous prefix) if they followed the script on its command line
    env["RBQ_BENCH_ARGV"] = json.dumps(sys.argv[1:])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)]
    print(f"[bench] --gpus {a.gpus}: launching {a.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode  # stdout is inherited: rank 0's JSON line goes straight through


def main():
    a = parse()
    if a.gpus > 1 and not a.in_library and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    import torch
    import torch.distributed as dist
    import rabitq_rs_amd as rq

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("RBQ_BENCH_REHEARSAL"):  # several ranks on ONE GPU with gloo: exercises the N>1 control flow only
        local = 0
    if a.gpus > 1 and not a.in_library and world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} under torch.distributed.run needs nproc-per-node {a.gpus} (WORLD_SIZE={world})")
    if a.in_library and world != 1:
        raise SystemExit("--in-library is ONE process with --gpus replicas inside one handle: do not start it under torch.distributed.run")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # RBQ_BENCH_FORCE_DIST: a process group even for ONE rank — the N > 1 code (RCCL init, the per-batch all_gather on the
    # batch's stream, barrier, all_reduce) then runs on a one-GPU box too (tests/test_gpu_parity.py)
    use_dist = world > 1 or bool(os.environ.get("RBQ_BENCH_FORCE_DIST"))
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if os.environ.get("RBQ_BENCH_REHEARSAL"):
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    # ---- pre-flight of an N-GPU run: every rank says which device it sits on, and rank 0 refuses to time
    # anything unless the N ranks hold N DISTINCT devices and the RCCL group has N members.  The process simply exits (non-zero):
    # nothing is re-executed, no GPU work has been queued yet.
    preflight = None
    if use_dist:
        props = torch.cuda.get_device_properties(dev)
        ident = f"{getattr(props, 'uuid', None) or ''}|pci={getattr(props, 'pci_bus_id', '?')}:{getattr(props, 'pci_device_id', '?')}|ordinal={local}"
        print(f"[bench preflight] rank {rank}/{world}: device ordinal {local}, {props.name}, {ident}", file=sys.stderr, flush=True)
        idents = [None] * world
        dist.all_gather_object(idents, ident if not os.environ.get("RBQ_BENCH_REHEARSAL") else f"{ident}|rank={rank}")
        distinct = len(set(idents))
        backend = dist.get_backend()
        preflight = {"ranks": world, "distinct_devices": distinct, "backend": backend, "group_size": dist.get_world_size(),
                     "rehearsal_on_one_gpu": bool(os.environ.get("RBQ_BENCH_REHEARSAL"))}
        ok = dist.get_world_size() == world and (distinct == world or world == 1)
        if not os.environ.get("RBQ_BENCH_REHEARSAL") and world > 1:
            ok = ok and backend == "nccl"
        if not ok:
            if rank == 0:
                print(f"[bench preflight] FAILED: {preflight} (identities: {idents})", file=sys.stderr, flush=True)
            dist.destroy_process_group()
            raise SystemExit(3)

    lib_devs = None
    if a.in_library:
        lib_devs = [0] * a.gpus if os.environ.get("RBQ_BENCH_REHEARSAL") else list(range(a.gpus))
        a.nbatches = max(a.nbatches, 2 * a.gpus)
        if a.device_build and not a.stream_build:
            a.stream_build = a.n  # the streamed builder is the device encoder that replicates (one chunk = the whole set)
    if world > 1 and not a.stream_build:
        a.device_build = True  # N ranks x an all-core CPU build on one host would only oversubscribe it; the
                               # device encoder produces the identical index (tests/test_gpu_parity.py)
    if a.stream_build:
        a.device_build = True
    full = a.full  # the supplementary legs run only on request; every flag below that trims them presupposes it
    extras = full and not a.no_extras and not a.ab and rank == 0
    stage_pass = full and (extras or a.ab) and rank == 0
    is_headline = all(getattr(a, k) == v for k, v in HEADLINE.items()) and a.dataset == "mixture_id32"

    def progress(msg):
        if rank == 0 and (a.device_build or a.n > 2_000_000):
            print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    def mark(msg):
        """one stderr line per leg of the run (rank 0): if a run dies, its log says where"""
        if rank == 0:
            print(f"[bench {time.strftime('%H:%M:%S')}] phase: {msg}", file=sys.stderr, flush=True)

    mix = Mixture(torch, dev, a.dim, a.nlist, a.dataset, a.metric == 1)
    NB = max(1, a.nbatches)
    nres = a.batch * a.top_k
    # every rank draws its own query batches from the same mixture (different streams per rank and batch)
    q_all = mix.draw(NB * a.batch, 20260102 + 7919 * rank).contiguous().view(NB, a.batch, a.dim)
    q_flat = q_all.view(NB * a.batch, a.dim)
    t_build0 = time.time()
    encoder = None
    built = None
    x = None

    def header_from_tiny_cpu_build(cent_h):
        # header (rotator flips, t_const) from a CPU build over a tiny subset: both depend only on (padded dim, bits, seed)
        ns_ = max(2 * a.nlist, 4096)
        xs = mix.draw(ns_, 99).cpu().numpy()
        return rq.builder.train_with_clusters(xs, cent_h, (np.arange(ns_) % a.nlist).astype(np.uint32), a.bits, a.metric,
                                              rq.RotatorType.FhtKacRotator, 20260104, True)

    if a.stream_build:
        # data never resident as a whole: chunk c of the base vectors is draw(chunk, 20260105 + c), regenerated per pass
        CH = a.stream_build
        nch = (a.n + CH - 1) // CH
        chunk = lambda c: mix.draw(min(CH, a.n - c * CH), 20260105 + c)  # noqa: E731
        sample = torch.cat([chunk(c)[:max(1, min(CH, 4_000_000 // nch))].clone() for c in range(nch)])  # (clone: a slice would pin its whole chunk)
        progress(f"k-means on a {sample.shape[0]}-vector sample")
        cent, _ = kmeans_gpu(torch, sample, a.nlist, a.kmeans_iters, 20260103)
        del sample
        cent_h = cent.cpu().numpy()
        small = header_from_tiny_cpu_build(cent_h)
        sizes = torch.zeros(a.nlist, dtype=torch.int64, device=dev)
        best = [torch.full((NB * a.batch, a.top_k), float("inf") if a.metric == 0 else float("-inf"), device=dev),
                torch.full((NB * a.batch, a.top_k), -1, dtype=torch.int64, device=dev)]
        assigns = []
        for c in range(nch):  # pass 1: assignment (count pass) + exact ground truth
            xc = chunk(c)
            ac = assign_gpu(torch, xc, cent).to(torch.int32)
            sizes += torch.bincount(ac, minlength=a.nlist)
            assigns.append(ac)
            exact_topk_update(torch, best, xc, c * CH, q_flat, a.top_k, a.metric)
            del xc
            if c % 8 == 0:
                progress(f"pass 1: chunk {c + 1}/{nch}")
        gt = best[1]
        torch.cuda.synchronize(dev)
        t0 = time.time()
        sb = rq.StreamBuilder(small.hdr_ptr, cent_h, sizes.cpu().numpy().astype(np.uint32), small.t_const, device=local)
        t_gen = 0.0
        for c in range(nch):  # pass 2: encode
            tg = time.time()
            xc = chunk(c)
            torch.cuda.synchronize(dev)
            t_gen += time.time() - tg
            sb.push(xc.data_ptr(), assigns[c].data_ptr(), c * CH, xc.shape[0])
            del xc
            if c % 8 == 0:
                progress(f"pass 2: chunk {c + 1}/{nch} pushed")
        idx = sb.finish(devices=lib_devs)
        t_enc_only = time.time() - t0 - t_gen
        del assigns
        progress(f"streamed encode done in {t_enc_only:.2f} s (+ {t_gen:.2f} s regenerating the chunks)")
        encoder = {"gpu_build_s": round(t_enc_only, 3), "vectors_per_s": a.n / t_enc_only, "chunk": CH, "chunks": nch,
                   "note": "--stream-build: rbq_build_stream_begin/push/finish, the raw vectors were never resident as a whole"}
        a.no_cpu = True
    else:
        x = mix.draw(a.n, 20260105)
        progress("data generated")
        cent, assign = kmeans_gpu(torch, x, a.nlist, a.kmeans_iters, 20260103)
        progress("clustered")
        if a.device_build:
            small = header_from_tiny_cpu_build(cent.cpu().numpy())
            a32 = assign.to(torch.int32).contiguous()
            torch.cuda.synchronize(dev)
            t0 = time.time()
            idx = rq.IvfRabitqIndex.build_on_device(small.hdr_ptr, cent.cpu().numpy(), x.data_ptr(), a32.data_ptr(), a.n,
                                                    small.t_const, device=local)
            t_enc_only = time.time() - t0
            progress(f"encoded in {t_enc_only:.2f} s")
            encoder = {"gpu_build_s": round(t_enc_only, 3), "vectors_per_s": a.n / t_enc_only, "arrays_identical_to_cpu_build": None,
                       "note": "--device-build: the index was built by rbq_index_build_device only"}
            a.no_cpu = True
        else:
            x_host = x.cpu().numpy()
            built = rq.builder.train_with_clusters(x_host, cent.cpu().numpy(), assign.cpu().numpy().astype(np.uint32), a.bits,
                                                   a.metric, rq.RotatorType.FhtKacRotator, 20260104, True)
            t_up0 = time.time()
            idx = rq.IvfRabitqIndex.from_built(built, device=local) if lib_devs is None else rq.IvfRabitqIndex.from_built(built, devices=lib_devs)
            t_upload = time.time() - t_up0
            del x_host
        gt = exact_topk(torch, x, q_flat, a.top_k, a.metric)
        progress("ground truth done")
    t_build = time.time() - t_build0

    # the same index from the GPU-side encoder (rbq_index_build_device): timed and compared array by array
    if built is not None and extras and a.bits in (1, 3, 7):
        a32 = assign.to(torch.int32).contiguous()
        cent_h = cent.cpu().numpy()
        torch.cuda.synchronize(dev)
        t0 = time.time()
        enc = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent_h, x.data_ptr(), a32.data_ptr(), a.n, built.t_const, device=local)
        t_enc = time.time() - t0
        ln = idx.debug_copy_index("list_n", np.empty(a.nlist, np.uint32))
        nslots = int(((ln + 31) // 32).sum()) * 32
        same = True
        for name, nb in (("ids", nslots * 8), ("fadd_ex", nslots * 4 if a.bits > 1 else 0), ("bsum", nslots)):
            if nb:
                same &= bool(np.array_equal(idx.debug_copy_index(name, np.empty(nb, np.uint8)),
                                            enc.debug_copy_index(name, np.empty(nb, np.uint8))))
        enc.close()
        encoder = {"gpu_build_s": round(t_enc, 3), "vectors_per_s": a.n / t_enc, "arrays_identical_to_cpu_build": same,
                   "upload_and_device_relayout_s": round(t_upload, 3),
                   "note": "rbq_index_build_device: rotate + quantize_with_centroid (faster config) + device layout, "
                           "clustering excluded; upload_and_device_relayout_s = rbq_index_create over the CPU build's "
                           "ClusterData (reference bytes uploaded, re-laid on the GPU)"}
    if not (extras and a.dataset == "mixture_id32" and is_headline):
        del x
    torch.cuda.empty_cache()

    for kv in a.option:
        k, v = kv.split("=")
        idx.set_option(k, int(v))

    D = idx.padded_dim
    Dc = (D + 63) // 64 * 64
    ex_bits = a.bits - 1

    def run_measured(index, qb, nprobe, steps, warmup, ns, gather, min_seconds=0.0):
        """run_timed() with the library's traffic counters OFF (the timed region is the product path: six atomics per query and
        the bookkeeping behind them cost it 2-3 %, 9 % before the counters were striped), then every distinct batch once more
        with the counters ON, untimed: the counts are deterministic per batch.  The stage timings (HIP events riding on the
        dispatch packets, free) come from the timed launches."""
        dts, own, prof = run_timed(index, qb, nprobe, steps, warmup, ns, gather, min_seconds, counters=False)
        _, _, pc = run_timed(index, qb, nprobe, int(qb.shape[0]), 0, ns, False, 0.0, counters=True, stages=("prep", "rank", "select", "scan"))
        prof["counters"], prof["algorithmic_bytes"], prof["counter_steps"] = pc["counters"], pc["algorithmic_bytes"], pc["steps_total"]
        prof["stage_ms_overlapped"] = pc["stage_ms"]  # every stage's mean duration while the batches overlap on ns streams
        return dts, own, prof

    def run_timed(index, qb, nprobe, steps, warmup, ns, gather, min_seconds=0.0, counters=True, stages=("scan",)):
        """Timed regions of exactly `steps` steps each (after `warmup` untimed steps), batches qb[NB'] rotating, on ns streams.
        Every region is bracketed by barrier + synchronize on both sides; regions repeat until `min_seconds` have been
        measured (a 20-step region lasts 4 ms: one sample of it is mostly noise).  Returns (region seconds — max over ranks —,
        this rank's own region seconds, profile over all regions)."""
        nbq = qb.shape[0]
        streams = [torch.cuda.Stream(dev) for _ in range(ns)]
        # Results go to 2 * ns slots = two buckets of ns consecutive batches.  A bucket is gathered by ONE all_gather (ns x
        # 123 KB per rank: fewer, larger collectives — the per-call cost of a collective is what a per-batch gather pays ns
        # times) on its own stream, behind the ns searches that fill it, while the search streams go on into the other bucket.
        nslots = 2 * ns
        ex = TopkExchange(torch, dev, a.batch, a.top_k, nslots, world, gather, single_rank_group=use_dist, bucket=ns)
        d_ids, d_sc, d_cnt = ex.ids, ex.scores, ex.counts
        counter = [0]
        xs = torch.cuda.Stream(dev) if ex.gathered is not None else None
        ev_search = [torch.cuda.Event() for _ in range(nslots)]
        ev_gathered = [None, None]
        pending = [0]  # searches enqueued since the last gather

        def gather_bucket(b):
            for slot in range(b * ns, (b + 1) * ns):
                xs.wait_event(ev_search[slot])
            with torch.cuda.stream(xs):
                ex.gather(dist, b)  # the path's only exchange: final top-k gather over RCCL/xGMI
                ev_gathered[b] = torch.cuda.Event()
                ev_gathered[b].record(xs)
            pending[0] = 0

        # the host's share of a step is part of the timed region (20 steps on 12 streams: the later streams start when their first
        # launch has been enqueued), so the per-step Python work is hoisted: device pointers and stream handles are looked up once
        fn_search = rq.index.lib().rbq_search_batch_device
        h_index = index._h
        q_ptrs = [t.data_ptr() for t in qb]
        out_ptrs = [(d_ids[k].data_ptr(), d_sc[k].data_ptr(), d_cnt[k].data_ptr()) for k in range(nslots)]
        stream_handles = [st.cuda_stream for st in streams]

        def step():
            i = counter[0]
            counter[0] += 1
            s, slot = i % ns, i % nslots
            if xs is not None and ev_gathered[slot // ns] is not None:
                streams[s].wait_event(ev_gathered[slot // ns])  # the bucket's previous contents have been gathered
            o = out_ptrs[slot]
            rc = fn_search(h_index, q_ptrs[i % nbq], a.batch, a.dim, a.top_k, nprobe, None, 0, o[0], o[1], o[2], None, stream_handles[s])
            if rc:
                raise RuntimeError(f"rbq_search_batch_device failed: {rc}")
            if xs is not None:
                ev_search[slot].record(streams[s])
                pending[0] += 1
                if slot % ns == ns - 1:
                    gather_bucket(slot // ns)

        def fence():
            if xs is not None and pending[0]:  # a partly filled bucket: its searches' results are exchanged too
                gather_bucket(((counter[0] - 1) % nslots) // ns)
            if gather and use_dist:
                dist.barrier()
            torch.cuda.synchronize(dev)

        torch.cuda.synchronize(dev)  # inputs were produced on the default stream
        for _ in range(ns):          # setup, not a warm-up step: every stream's workspace is allocated on its first call
            step()
        fence()
        for _ in range(warmup):
            step()
        fence()
        # HIP events on the kernels' own stream, no host sync inside the timed region.  Only the roofline kernel is
        # timed here (the event pair rides on the dispatch packet); about 25 launches per region are sampled.  The traffic
        # counters run on every launch (one atomicAdd per workgroup at exit).
        index.set_option("profile_counters", 1 if counters else 0)
        if True:
            index.profile_begin(stages=stages, every=int(os.environ.get("RBQ_BENCH_TAP_EVERY", str(max(1, steps // 25)))))
        dts, own, t_issue = [], [], 0.0
        while True:
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            t_issue += time.perf_counter() - t0  # host time to enqueue the region's work (no wait in it)
            fence()
            dt = time.perf_counter() - t0
            own.append(dt)
            if gather and use_dist:  # max over ranks (outside the timed bracket); identical on every rank afterwards
                t = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            dts.append(dt)
            if sum(dts) >= min_seconds or len(dts) >= 64:
                break
        last = counter[0] - 1  # the last timed step: its batch and the result slot it wrote (synchronized by fence())
        last_out = {"ids": d_ids[last % nslots], "scores": d_sc[last % nslots], "counts": d_cnt[last % nslots], "batch": last % nbq}
        index.profile_end()
        index.set_option("profile_counters", 1)
        nreg = len(dts)
        ms, launches = index.profile_stage("scan")
        prof = {"issue_s": t_issue / nreg, "scan_ms": ms, "scan_launches": launches, "scan_samples_ms": [round(float(v), 4) for v in index.profile_stage_samples("scan")][:64],
                "counters": index.profile_counters(), "steps_total": steps * nreg, "counter_steps": steps * nreg,
                "algorithmic_bytes": index.profile_scan_bytes(),
                "stage_ms": {st_: index.profile_stage(st_)[0] for st_ in stages}, "last_out": last_out}
        for st in streams:
            index.release_stream(st.cuda_stream)
        return dts, own, prof

    def search_ids(index, qb, nprobe):
        """ids [nb][batch][top_k] of the given batches (one stream, synchronous)"""
        out = []
        st = torch.cuda.Stream(dev)
        d_ids = torch.empty(a.batch, a.top_k, dtype=torch.int64, device=dev)
        d_sc = torch.empty(a.batch, a.top_k, dtype=torch.float32, device=dev)
        d_cnt = torch.empty(a.batch, dtype=torch.int32, device=dev)
        for b in range(qb.shape[0]):
            index.search_batch_device(qb[b].data_ptr(), a.batch, a.dim, a.top_k, nprobe, d_ids.data_ptr(), d_sc.data_ptr(),
                                      d_cnt.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            out.append(d_ids.cpu().numpy().view(np.uint64).copy())
        index.release_stream(st.cuda_stream)
        return np.stack(out)

    def lists_scanned(index, qbatch):
        """mean number of probed lists that reach k_scan (the others are provably skipped as a whole by the lazy selection)"""
        st = torch.cuda.Stream(dev)
        d_i = torch.empty(a.batch, a.top_k, dtype=torch.int64, device=dev)
        d_s = torch.empty(a.batch, a.top_k, dtype=torch.float32, device=dev)
        d_c = torch.empty(a.batch, dtype=torch.int32, device=dev)
        index.search_batch_device(qbatch.data_ptr(), a.batch, a.dim, a.top_k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        try:
            ds = index.debug_copy_workspace(st.cuda_stream, "dead_skipped", np.empty((2, a.batch), np.uint32))
            out_ = float(ds[1].mean())
        except Exception:  # noqa: BLE001
            out_ = None
        index.release_stream(st.cuda_stream)
        return out_

    def pruned_object(prof, steps):
        c = prof["counters"]
        req, parts = traffic_of(c, D, Dc, ex_bits, steps)
        alg = prof["algorithmic_bytes"] / max(steps, 1)
        ms = prof["scan_ms"]
        return {"kernel": "the scan of the product configuration (exact block-level bound ON; which kernel: regime.scan_kernel)",
                "avg_launch_ms": ms, "launches": prof["scan_launches"],
                "algorithmic_bytes_per_launch": alg, "bytes_requested_per_launch": req, "bytes_requested_by_array": parts,
                "algorithmic_bytes_are": "of the APPROXIMATE probe set (the lazy selection resolves the boundary zone of the nprobe-th score only "
                                         "when a list in it is alive; within 2 % of the exact figure, which `roofline` — eager selection — carries)",
                # probed blocks whose codes were never fetched (vectors_probed / 32: lists proved skipped as a whole by the probe
                # selection never enter the stream, so the stream-entry count is no longer the number of probed blocks)
                "block_skip_frac": 1.0 - c["code_blocks"] / max(c["vectors_probed"] / 32.0, 1.0),
                "stream_entries_per_launch": c["stream_entries"] / max(steps, 1),
                "frac": req / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS if ms > 0 else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "algorithmic_over_time_GBs": alg / (ms * 1e-3) / 1e9 if ms > 0 else None,
                "counters_from": "an untimed pass over the same query batches with the library's traffic counters on (deterministic per "
                                 "batch); the timed region runs without them; avg_launch_ms = HIP events on the timed launches",
                "note": "bytes_requested = what the kernel asked the memory system for in these launches (its own counters: "
                        "sign-code records, factor rows, 16-byte stream entries, ex codes of refined candidates, per-query LUT "
                        "and rotated query); provably pruned blocks are never fetched, so the algorithmic bytes are NOT moved "
                        "and algorithmic_over_time is not a bandwidth"}

    def pinned_sets(per_call, nsets, nthr=1):
        """page-locked (rbq_host_alloc) query / ids / scores / counts buffers, one set per (thread, query set)"""
        import ctypes as C
        lib = rq.index.lib()
        nbytes = [per_call * a.dim * 4, per_call * a.top_k * 8, per_call * a.top_k * 4, per_call * 4]
        pin = [[[lib.rbq_host_alloc(b) for b in nbytes] for _ in range(nsets)] for _ in range(nthr)]
        for j in range(nsets):
            off = (j * per_call) % max(NB * a.batch - per_call + 1, 1)
            qh = q_flat[off:off + per_call].cpu().numpy()
            for t in range(nthr):
                C.memmove(pin[t][j][0], qh.ctypes.data, nbytes[0])
        return pin, nbytes

    def free_sets(pin):
        lib = rq.index.lib()
        for a_ in pin:
            for b_ in a_:
                for p_ in b_:
                    lib.rbq_host_free(p_)

    def latency_leg():
        """p50 / p99 of ONE rbq_search_batch call (page-locked host buffers in and out) at small nq — `search` (nq = 1,
        src/ivf.rs:1705-1711) is the reference's primary API and what its published numbers time in a sequential loop
        (examples/recall_qps_sweep.rs:127-138)."""
        lib = rq.index.lib()
        res = {}
        for nq_ in (1, 4, 8, 64, 256):
            if nq_ > NB * a.batch:
                continue
            nsets = 16 if nq_ <= 64 else 8
            pin, _ = pinned_sets(nq_, nsets)
            call = lambda j: lib.rbq_search_batch(idx._h, pin[0][j][0], nq_, a.dim, a.top_k, a.nprobe, None, 0, pin[0][j][1], pin[0][j][2], pin[0][j][3], None)  # noqa: E731
            for j in range(nsets):
                assert call(j) == 0
            reps = 200 if nq_ <= 64 else 100
            ts = []
            for r in range(reps):
                t0 = time.perf_counter()
                rc = call(r % nsets)
                ts.append(time.perf_counter() - t0)
                assert rc == 0
            ts = np.array(ts) * 1e6
            res[str(nq_)] = {"p50_us": round(float(np.percentile(ts, 50)), 1), "p99_us": round(float(np.percentile(ts, 99)), 1),
                             "mean_us": round(float(ts.mean()), 1), "queries_per_s_sequential_calls": nq_ / (float(ts.mean()) * 1e-6), "calls": reps}
            if nq_ in (1, 64):  # the same calls through the batch kernels (k_prep_wave + GEMM): what the latency-first path (latency.hpp) buys
                idx.set_option("latency_path", 0)
                for j in range(nsets):
                    call(j)
                t2 = []
                for r in range(reps):
                    t0 = time.perf_counter()
                    call(r % nsets)
                    t2.append(time.perf_counter() - t0)
                idx.set_option("latency_path", 1)
                res[str(nq_)]["p50_us_batch_kernels"] = round(float(np.percentile(np.array(t2) * 1e6, 50)), 1)
            free_sets(pin)
        res["path"] = ("calls of up to 4 queries: k_lat_front (rotation + constants + LUT + the exact score of every list, one launch) + selection + "
                       "scan; up to 512 queries: the preparation with a workgroup per query; p50_us_batch_kernels = option latency_path = 0")
        res["note"] = ("one caller thread, one call at a time, distinct queries per call, page-locked buffers (rbq_host_alloc); "
                       "includes H2D of the queries, the four kernels and the results written to host memory. Context only: the "
                       "reference publishes sequential single-query numbers on its own hardware "
                       "(benchmarks/gist_1m_results/recall_qps_fixed.csv)")
        return res

    if a.in_library:
        # ---- ONE process, ONE handle with a.gpus replicas: a step = one rbq_search_batch call over gpus x batch queries in
        # page-locked host buffers (weak scaling: `batch` queries per replica and step), results into host buffers
        import ctypes as C
        import threading
        lib = rq.index.lib()
        per_call = a.batch * a.gpus
        nthr = max(1, a.caller_threads)
        nsets = max(2, min(8, NB * a.batch // per_call))
        pin, nbytes = pinned_sets(per_call, nsets, nthr)

        def worker(t, n):
            for r in range(n):
                pp = pin[t][(t + r) % nsets]
                rc_ = lib.rbq_search_batch(idx._h, pp[0], per_call, a.dim, a.top_k, a.nprobe, None, 0, pp[1], pp[2], pp[3], None)
                assert rc_ == 0, rc_

        def region(n):
            share = [n // nthr + (1 if t < n % nthr else 0) for t in range(nthr)]
            th = [threading.Thread(target=worker, args=(t, share[t])) for t in range(1, nthr)]
            t0 = time.perf_counter()
            for t_ in th:
                t_.start()
            worker(0, share[0])
            for t_ in th:
                t_.join()
            return time.perf_counter() - t0

        region(max(a.warmup, 2 * nthr))
        dts = []
        while True:
            dts.append(region(a.steps))
            if sum(dts) >= a.min_seconds or len(dts) >= 64:
                break
        dt = statistics.median(dts)
        value = per_call * a.steps / dt
        if a.dump_outputs:  # the last call of caller thread 0 in the last region (worker 0 makes share[0] calls, query set r % nsets)
            pp = pin[0][(a.steps // nthr + (1 if a.steps % nthr else 0) - 1) % nsets]
            host = lambda p_, ct, shape: np.ctypeslib.as_array(C.cast(p_, C.POINTER(ct)), shape=shape).copy()  # noqa: E731
            dump_outputs(a.dump_outputs, host(pp[1], C.c_uint64, (per_call, a.top_k)), host(pp[2], C.c_float, (per_call, a.top_k)),
                         host(pp[3], C.c_uint32, (per_call,)), host(pp[0], C.c_float, (per_call, a.dim)))
        # results of the first query set against the exact ground truth, and against ONE replica serving the same queries
        ids0 = np.ctypeslib.as_array(C.cast(pin[0][0][1], C.POINTER(C.c_uint64)), shape=(per_call, a.top_k)).copy()
        gtn = gt.cpu().numpy()[:per_call]
        recall = recall_of(ids0, gtn, a.top_k)
        d_i = torch.empty(per_call, a.top_k, dtype=torch.int64, device=dev)
        d_s = torch.empty(per_call, a.top_k, dtype=torch.float32, device=dev)
        d_c = torch.empty(per_call, dtype=torch.int32, device=dev)
        idx.search_batch_device(q_flat[:per_call].contiguous().data_ptr(), per_call, a.dim, a.top_k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(),
                                d_c.data_ptr(), stream=None)
        torch.cuda.synchronize(dev)
        same = bool(np.array_equal(d_i.cpu().numpy().view(np.uint64), ids0))
        what = f"N={a.n} d={a.dim}, nlist={a.nlist}, {a.bits}-bit, FhtKacRotator, {'L2' if a.metric == 0 else 'IP'}, nprobe={a.nprobe}, " \
               f"top_k={a.top_k}, batch={a.batch} per GPU"
        out = {"metric": f"queries/sec at recall@{a.top_k}={recall:.3f}, in-library replicas, host buffers, synthetic {a.dataset} {what}",
               "value": value, "unit": "queries/s", "n_gpus": a.gpus, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
               "config": {"workload": f"synthetic GIST-1M-shaped fvecs ({a.dataset}) {what}",
                          "parallelism": f"in-library: ONE process, ONE rbq_index with {a.gpus} replicas on devices {lib_devs}; every step is one "
                                         f"rbq_search_batch call over {per_call} queries in page-locked host buffers, sharded over the replicas",
                          "caller_threads": nthr, "distinct_query_sets": nsets, "timed_regions": len(dts),
                          "value_is": "host-buffer rate (H2D of the queries and results in host memory included)"},
               "region_ms": [round(v * 1e3, 3) for v in dts],
               f"recall_at_{a.top_k}": recall, "recall_ok": recall >= 0.95,
               "ids_identical_to_one_replica_device_entry": same,
               "replicas": int(idx.device_count()), "rank_fallbacks": int(idx.rank_fallbacks()), "heap_restarts": int(idx.heap_restarts()),
               # how replica 0's arrays reached the other replicas: hipMemcpyPeer, or the page-locked bounce buffer when the runtime
               # refuses peer access (rbq_debug_bounce_copies counts the latter); and what the runtime says about peer access
               "replica_copy": "bounce" if int(rq.index.lib().rbq_debug_bounce_copies()) > 0 else ("peer" if a.gpus > 1 else "none"),
               "peer_access": [[bool(i == j or (lib_devs[i] != lib_devs[j] and torch.cuda.can_device_access_peer(lib_devs[i], lib_devs[j])))
                                for j in range(a.gpus)] for i in range(a.gpus)] if a.gpus > 1 else None,
               "latency": None if a.no_latency else latency_leg(),
               "roofline": None, "cpu_baseline": None}
        free_sets(pin)
        print(json.dumps(out))
        return

    mark("timed regions + counter pass" if full else "timed regions")
    ns = max(1, a.streams)
    if full:
        dts, own_dts, prof = run_measured(idx, q_all, a.nprobe, a.steps, a.warmup, ns, gather=True, min_seconds=a.min_seconds)
    else:  # the same timed regions, without the untimed counter pass behind them
        dts, own_dts, prof = run_timed(idx, q_all, a.nprobe, a.steps, a.warmup, ns, True, a.min_seconds, counters=False)
    last = prof.pop("last_out")
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last["ids"].cpu().numpy().view(np.uint64), last["scores"].cpu().numpy(),
                     last["counts"].cpu().numpy().view(np.uint32), q_all[last["batch"]].cpu().numpy())
    dt = statistics.median(dts)  # the median K-step region (each one bracketed by barrier + synchronize, max over ranks)
    value = a.batch * world * a.steps / dt
    per_rank = [a.batch * a.steps / statistics.median(own_dts)]
    rccl_world = None
    if use_dist:
        t = torch.zeros(world, device=dev, dtype=torch.float64)
        t[rank] = per_rank[0]
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        per_rank = [float(v) for v in t.tolist()]
        rccl_world = dist.get_world_size() if dist.get_backend() == "nccl" else None

    mark("results of every batch (recall)")
    # results of every batch (one stream): recall over ALL of them, and the same ids whatever the stream
    ids_all = search_ids(idx, q_all, a.nprobe)
    gtn = gt.cpu().numpy().reshape(NB, a.batch, a.top_k)
    recall = recall_of(ids_all.reshape(-1, a.top_k), gtn.reshape(-1, a.top_k), a.top_k)
    pruned = pruned_object(prof, prof["counter_steps"]) if full else None

    # the roofline figure: the same kernel with the block-level bound switched off streams EVERY probed block — the
    # algorithmic bytes are really moved (results identical, only the work changes); one stream, k_scan alone on the chip
    if full:
        mark("roofline leg (block bound off) + per-stage pass")
    roofline = None
    serial = None
    if rank == 0 and full:
        n_rf = max(6, min(a.steps // 4, 50))
        idx.set_option("block_bound", 0)
        _, _, p2 = run_timed(idx, q_all, a.nprobe, n_rf, 2, 1, gather=False)
        ids_off = search_ids(idx, q_all[:2], a.nprobe)
        # the same streaming configuration through the wave-per-query kernel (k_scanw: what serves the PRUNED regime of this batch
        # size; the library picks k_scan when every block is streamed)
        wave = None
        try:
            if a.no_wave_roofline:
                raise RuntimeError("skipped (--no-wave-roofline)")
            idx.set_option("scan_wave", 1)
            _, _, p3 = run_timed(idx, q_all, a.nprobe, n_rf, 2, 1, gather=False)
            ids_w = search_ids(idx, q_all[:2], a.nprobe)
            ach3 = p3["algorithmic_bytes"] / n_rf / (p3["scan_ms"] * 1e-3) / 1e9
            wave = {"kernel": "k_scanw (one wave per query)", "achieved": ach3, "frac": ach3 / HBM_PEAK_GBS, "avg_launch_ms": p3["scan_ms"],
                    "launches": p3["scan_launches"], "ids_identical_to_product_configuration": bool(np.array_equal(ids_w, ids_all[:2]))}
        except Exception as e:  # noqa: BLE001
            wave = {"error": str(e)[:200]}
        idx.set_option("scan_wave", -1)
        idx.set_option("block_bound", 1)
        alg2 = p2["algorithmic_bytes"] / n_rf
        req2, _ = traffic_of(p2["counters"], D, Dc, ex_bits, n_rf)
        ach = alg2 / (p2["scan_ms"] * 1e-3) / 1e9
        roofline = {"bound": "hbm", "kernel": "k_scan (one workgroup per query: the kernel the library runs when every probed block is streamed)",
                    "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": ach / HBM_PEAK_GBS, "traffic": PMC_TRAFFIC.get("bytes") if is_headline else None,
                    "traffic_from": PMC_TRAFFIC.get("source") if is_headline else None,
                    "algorithmic_bytes_per_launch": alg2, "bytes_requested_per_launch": req2, "avg_launch_ms": p2["scan_ms"],
                    "launches": p2["scan_launches"], "launch_ms": p2["scan_samples_ms"], "ids_identical_to_product_configuration": bool(np.array_equal(ids_off, ids_all[:2])),
                    "wave_kernel_same_configuration": wave,
                    "configuration": "block-level bound OFF (rbq_debug_set_option block_bound=0): every probed block is streamed, "
                                     "so the algorithmic bytes (SURVEY 8d: sum n_c*(D/8+12)) are the bytes moved; one stream, "
                                     "distinct query batch per launch; HIP events carried by the dispatch packets",
                    "note": "traffic = FETCH_SIZE x 2 of the committed PMC pass of this build (profiles/r5/summary_headline.md; null when no pass "
                            "exists for the configuration); bytes_requested_per_launch is the kernel's own count for the same launches "
                            "(codes + factor rows + stream + ex codes + LUT)"}
        if stage_pass:
            # every stage alone on one stream (no overlap between batches), rotating batches
            stv = torch.cuda.Stream(dev)
            d_i = torch.empty(a.batch, a.top_k, dtype=torch.int64, device=dev)
            d_s = torch.empty(a.batch, a.top_k, dtype=torch.float32, device=dev)
            d_c = torch.empty(a.batch, dtype=torch.int32, device=dev)
            n_ser = max(5, min(a.steps // 2, 64))
            for phase in range(2):
                if phase == 1:
                    idx.profile_begin()
                for i in range(2 if phase == 0 else n_ser):
                    idx.search_batch_device(q_all[i % NB].data_ptr(), a.batch, a.dim, a.top_k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(),
                                            d_c.data_ptr(), stream=stv.cuda_stream)
                torch.cuda.synchronize(dev)
            idx.profile_end()
            sm = {s: idx.profile_stage(s) for s in ("prep", "rank", "select", "scan")}
            serial = {"stage_ms": {k: round(v[0], 4) for k, v in sm.items()}, "launches": sm["scan"][1]}
            idx.release_stream(stv.cuda_stream)
    if use_dist:
        dist.barrier()

    # the host-buffer entry point (rbq_search_batch: H2D of the queries, the four kernels, D2H of the results) — what a
    # CPU-side caller such as the Rust shim binds (src/ivf.rs:1743-1752)
    if full:
        mark("host entry legs")
    pcie = None
    host_call = None
    if extras:
        import ctypes as C
        import threading
        lib = rq.index.lib()
        nthr = 4

        def host_leg(per_call):
            """rates of rbq_search_batch with `per_call` queries per call (per_call = k * batch: k query batches back to back)"""
            kb = per_call // a.batch
            nsets = max(2, min(8, NB // kb))
            qh = [q_all[(j * kb) % NB:(j * kb) % NB + kb].reshape(per_call, a.dim).cpu().numpy() for j in range(nsets)]
            sp = rq.SearchParams(a.top_k, a.nprobe)
            hid = idx.batch_search_raw(qh[0], sp)[0]
            nbytes = [per_call * a.dim * 4, per_call * a.top_k * 8, per_call * a.top_k * 4, per_call * 4]
            # page-locked buffers (rbq_host_alloc): one set per thread and query set
            pin = [[[lib.rbq_host_alloc(b) for b in nbytes] for _ in range(nsets)] for _ in range(nthr)]
            for t in range(nthr):
                for j, qq in enumerate(qh):
                    C.memmove(pin[t][j][0], qq.ctypes.data, nbytes[0])

            def timed(fn, nthreads, nrep, tries=3):
                best = 0.0
                for _ in range(tries):  # best of 3: the box shares its host CPUs (cgroup quota), single runs scatter
                    th = [threading.Thread(target=fn, args=(t, nrep)) for t in range(nthreads)]
                    t0 = time.perf_counter()
                    for t in th:
                        t.start()
                    for t in th:
                        t.join()
                    best = max(best, per_call * nthreads * nrep / (time.perf_counter() - t0))
                return best

            def pageable(t, nrep):
                for r in range(nrep):
                    idx.batch_search_raw(qh[(t * 3 + r) % nsets], sp)

            def pinned(t, nrep):
                for r in range(nrep):
                    p = pin[t][(t * 3 + r) % nsets]
                    rc = lib.rbq_search_batch(idx._h, p[0], per_call, a.dim, a.top_k, a.nprobe, None, 0, p[1], p[2], p[3], None)
                    assert rc == 0

            def per_call_times(fn, ncalls):
                """ONE caller thread, one call at a time: seconds of each of `ncalls` calls (distinct query sets in rotation)"""
                ts = np.empty(ncalls)
                for r in range(ncalls):
                    t0 = time.perf_counter()
                    fn(r)
                    ts[r] = time.perf_counter() - t0
                return ts

            def one_pageable(r):
                idx.batch_search_raw(qh[r % nsets], sp)

            def one_pinned(r):
                p = pin[0][r % nsets]
                assert lib.rbq_search_batch(idx._h, p[0], per_call, a.dim, a.top_k, a.nprobe, None, 0, p[1], p[2], p[3], None) == 0

            timed(pageable, 1, 3, 1)
            timed(pinned, 1, 3, 1)
            reps = max(10, 64 * a.batch // per_call)  # calls per thread and try (a few tens of ms: thread start-up does not weigh)
            want = ids_all[:kb].reshape(per_call, a.top_k)
            ncalls = max(40, 200 * a.batch // per_call)
            tp_, tg_ = per_call_times(one_pinned, ncalls), per_call_times(one_pageable, ncalls)
            leg = {"queries_per_call": per_call,
                   # the robust single-caller figures: MEDIAN call (the box shares its host CPUs; best-of-N flatters)
                   "calls_timed": ncalls,
                   "page_locked_us_per_call": {"median": float(np.median(tp_) * 1e6), "p10": float(np.percentile(tp_, 10) * 1e6), "p90": float(np.percentile(tp_, 90) * 1e6)},
                   "pageable_us_per_call": {"median": float(np.median(tg_) * 1e6), "p10": float(np.percentile(tg_, 10) * 1e6), "p90": float(np.percentile(tg_, 90) * 1e6)},
                   "page_locked_queries_per_s": per_call / float(np.median(tp_)),
                   "pageable_queries_per_s": per_call / float(np.median(tg_)),
                   "queries_per_s_1_caller_thread": timed(pageable, 1, reps),
                   f"queries_per_s_{nthr}_caller_threads": timed(pageable, nthr, reps),
                   "pinned_queries_per_s_1_caller_thread": timed(pinned, 1, reps),
                   f"pinned_queries_per_s_{nthr}_caller_threads": timed(pinned, nthr, reps),
                   "ids_identical_to_device_path": bool(np.array_equal(hid, want)),
                   "pinned_ids_identical": bool(np.array_equal(
                       np.ctypeslib.as_array(C.cast(pin[0][0][1], C.POINTER(C.c_uint64)), shape=(per_call, a.top_k)), want)),
                   "bytes_per_call": {"h2d": nbytes[0], "d2h": nbytes[1] + nbytes[2] + nbytes[3]}}
            leg["over_device_resident_1_thread"] = leg["queries_per_s_1_caller_thread"] / (value / world)
            leg["pinned_over_device_resident_1_thread"] = leg["pinned_queries_per_s_1_caller_thread"] / (value / world)
            for t in range(nthr):
                for j in range(nsets):
                    for p in pin[t][j]:
                        lib.rbq_host_free(p)
            return leg

        pcie = {"per_call_1x_batch": host_leg(a.batch)}
        if NB >= 8:
            pcie["per_call_4x_batch"] = host_leg(4 * a.batch)
        # The call the reference binds, first-class: batch_search(&[&[f32]], params) (src/ivf.rs:1743-1752) = ONE rbq_search_batch
        # call per step from ONE caller thread, host slices in, host vectors out, distinct batches.  `value` stays the
        # device-resident rate (the bench contract: inputs resident in HBM when the timed region starts); this object is what a
        # Rust / Python caller of the drop-in sees.
        l1 = pcie["per_call_1x_batch"]
        host_call = {"what": "rbq_search_batch: host buffers in and out, ONE caller thread, ONE call per step, distinct batches; median call of "
                             f"{l1['calls_timed']} (the reference's batch_search binding, src/ivf.rs:1743-1752)",
                     "queries_per_call": a.batch,
                     "queries_per_s": l1["page_locked_queries_per_s"], "buffers": "page-locked (rbq_host_alloc)",
                     "us_per_call": l1["page_locked_us_per_call"],
                     "pageable_queries_per_s": l1["pageable_queries_per_s"], "pageable_us_per_call": l1["pageable_us_per_call"],
                     "over_device_resident": l1["page_locked_queries_per_s"] / (value / world),
                     "ids_identical_to_device_path": l1["pinned_ids_identical"] and l1["ids_identical_to_device_path"],
                     "bound": "one call = the time the GPU needs for `queries_per_call` queries at its pipelined rate (1 / device-resident rate) "
                              "+ the latency of ONE four-kernel chain (latency.p50 of a small call): the sub-batches of a call overlap like the "
                              "device-resident batches do, but nothing overlaps the first chain's fill and the last chain's drain",
                     "model_us_per_call": None}
        if "per_call_4x_batch" in pcie:
            l4 = pcie["per_call_4x_batch"]
            host_call["per_call_4x_batch"] = {"queries_per_call": l4["queries_per_call"], "queries_per_s": l4["page_locked_queries_per_s"],
                                              "pageable_queries_per_s": l4["pageable_queries_per_s"], "us_per_call": l4["page_locked_us_per_call"]}
        pcie["note"] = ("rbq_search_batch, host buffers in and out, distinct batches per call, best of 3 runs per figure; default rows = pageable numpy buffers "
                        "(staged through the handle's pinned memory), pinned_* rows = caller buffers from rbq_host_alloc (DMA-ed / "
                        "written directly).  One call of one batch is bound by the serial latency of its four kernels + the H2D copy; "
                        "calls of several batches (sub-batches pipelined over the handle's lanes) and concurrent caller threads "
                        "approach the device-resident rate.  `value` is the device-resident rate; these are the rates a host-side "
                        "caller sees.")

    if full:
        mark("latency leg")
    latency = latency_leg() if (extras and not a.no_latency) else None
    if host_call is not None and latency is not None and "64" in latency:
        host_call["model_us_per_call"] = a.batch / (value / world) * 1e6 + latency["64"]["p50_us"]

    # Self-check for indexes no CPU oracle run can cover (device-built: cfg5 at 100 M vectors): the first 256 queries again
    # with every shortcut switched off — canonical all-pairs ranking instead of the MFMA shortlist, BinaryHeap emulation from
    # the first candidate, no block-level bound — must give the same bits.
    if full:
        mark("self check")
    self_check = None
    if extras:
        nsc = min(256, a.batch)
        qs_ = q_all[0][:nsc].contiguous()
        def run_sc():
            d_i = torch.empty(nsc, a.top_k, dtype=torch.int64, device=dev)
            d_s = torch.empty(nsc, a.top_k, dtype=torch.float32, device=dev)
            d_c = torch.empty(nsc, dtype=torch.int32, device=dev)
            st_ = torch.cuda.Stream(dev)
            idx.search_batch_device(qs_.data_ptr(), nsc, a.dim, a.top_k, a.nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st_.cuda_stream)
            st_.synchronize()
            idx.release_stream(st_.cuda_stream)
            return d_i.cpu().numpy(), d_s.cpu().numpy().view(np.uint32), d_c.cpu().numpy()
        fast = run_sc()
        for k_, v_ in (("exact_rank", 1), ("exact_heap", 1), ("block_bound", 0)):
            idx.set_option(k_, v_)
        slow = run_sc()
        for k_, v_ in (("exact_rank", 0), ("exact_heap", 0), ("block_bound", 1)):
            idx.set_option(k_, v_)
        self_check = {"queries": nsc, "ids_identical": bool(np.array_equal(fast[0], slow[0])), "score_bits_identical": bool(np.array_equal(fast[1], slow[1])),
                      "counts_identical": bool(np.array_equal(fast[2], slow[2])),
                      "against": "the same queries with exact_rank=1 (canonical all-pairs centroid ranking), exact_heap=1 (BinaryHeap emulation from the "
                                 "first candidate) and block_bound=0 (every probed block scanned)"}

    # second data set of the pair (rank 0, headline workload only): SURVEY 8d's isotropic mixture
    datasets = None
    if full:
        mark("second data set")
        datasets = {a.dataset: {"recall_at_k": recall, "queries_per_s": value / world, "nprobe": a.nprobe,
                                "block_skip_frac": pruned["block_skip_frac"], "role": "headline"}}
    if extras and is_headline:
        del x
        torch.cuda.empty_cache()
        iso = Mixture(torch, dev, a.dim, a.nlist, "isotropic", False)
        xi = iso.draw(a.n, 20260105)
        ci, ai = kmeans_gpu(torch, xi, a.nlist, a.kmeans_iters, 20260103)
        hdr_src = built if built is not None else small
        idx2 = rq.IvfRabitqIndex.build_on_device(hdr_src.hdr_ptr, ci.cpu().numpy(), xi.data_ptr(), ai.to(torch.int32).contiguous().data_ptr(),
                                                 a.n, hdr_src.t_const, device=local)
        nb2 = min(NB, 8)
        qi = iso.draw(nb2 * a.batch, 20260102).contiguous().view(nb2, a.batch, a.dim)
        gti = exact_topk(torch, xi, qi.view(-1, a.dim), a.top_k, a.metric).cpu().numpy()
        del xi
        torch.cuda.empty_cache()
        rows, reached = [], None
        for npb in (a.nprobe, 2 * a.nprobe, 4 * a.nprobe):
            dti, _, pi = run_timed(idx2, qi, npb, 24, 4, ns, gather=False)
            dti = dti[0]
            ri = recall_of(search_ids(idx2, qi, npb).reshape(-1, a.top_k), gti, a.top_k)
            po = pruned_object(pi, 24)
            rows.append({"nprobe": npb, "recall_at_k": ri, "queries_per_s": a.batch * 24 / dti, "block_skip_frac": po["block_skip_frac"],
                         "bytes_requested_per_launch": po["bytes_requested_per_launch"]})
            if reached is None and ri >= 0.95:
                reached = npb
        datasets["isotropic"] = {"role": "SURVEY 8d recipe (x = mean_k + 0.35 N(0, I_d)); reported beside the headline, never the headline",
                                 "by_nprobe": rows, "smallest_nprobe_reaching_recall_0.95": reached,
                                 "note": "isotropic noise in d=960 leaves the 10 nearest neighbours equidistant to a few per cent; the "
                                         "reference's estimator itself cannot separate them (DESIGN.md)"}
        idx2.close()

    # What bounds the TIMED configuration.  It is not HBM (97 % of the probed blocks are provably pruned: `pruned`) and not issue
    # slots: every kernel of the path is a chain of dependent phases per query, so the chip fills with resident waves that
    # wait.  Per stage: the kernel instantiation this call shape launches and what it occupies (rbq_debug_stage_resources: live,
    # from the code object), its duration alone and under overlap (HIP events on the dispatch packets); resident wave-time per
    # step against the wave slots the chip offers in one step time.
    if full:
        mark("regime + sensitivity")
    regime = None
    if rank == 0 and full:
        try:
            res = idx.stage_resources(a.batch, a.top_k, a.nprobe)
        except Exception as e:  # noqa: BLE001
            res = None
            progress(f"stage_resources failed: {e}")
        if res is not None:
            SIMDS, VGPR_FILE, LDS_CU, MAX_WAVES = 1024, 512, 160 * 1024, 8
            ov = prof.get("stage_ms_overlapped") or {}
            step_ms = dt / a.steps * 1e3
            stages_o, wave_ms, slot_ms = {}, 0.0, 0.0
            for st_, r_ in res.items():
                wpw = max(r_["threads"] // 64, 1)
                waves = r_["workgroups"] * wpw
                by_vgpr = min(MAX_WAVES, VGPR_FILE // max(8, (r_["vgprs"] + 7) // 8 * 8))
                wg_per_cu = (by_vgpr * 4) // wpw
                if r_["lds_bytes"]:
                    wg_per_cu = min(wg_per_cu, LDS_CU // r_["lds_bytes"])
                waves_per_simd = max(1, min(by_vgpr, wg_per_cu * wpw // 4))
                d_al = serial["stage_ms"].get(st_) if serial else None
                stages_o[st_] = dict(r_, waves=waves, waves_per_simd_by_registers=by_vgpr, waves_per_simd=waves_per_simd,
                                     ms_alone=d_al, ms_overlapped=ov.get(st_))
                if d_al:
                    wave_ms += waves * d_al
                    slot_ms += waves * d_al / waves_per_simd  # SIMD-milliseconds: the stage's waves at its own occupancy limit
            regime = {"bound": "residency / latency: dependent phases per query keep waves resident while they wait; neither HBM "
                               "(see `pruned`) nor issue slots",
                      "stages": stages_o,
                      # the product configuration's scan: 64 threads per query = k_scanw (one wave per query), 256 = k_scan
                      "scan_kernel": ("k_scanw (one wave per query)" if (res.get("scan") or {}).get("threads") == 64 else "k_scan (one workgroup of four waves per query)"),
                      "ms_per_step": step_ms,
                      "sum_of_stage_ms_alone": (sum(v for v in serial["stage_ms"].values()) if serial else None),
                      "overlap_gain": (sum(v for v in serial["stage_ms"].values()) / step_ms if serial else None),
                      "resident_wave_us_per_query_upper": wave_ms * 1e3 / a.batch if wave_ms else None,
                      "residency_model_ms_per_step": slot_ms / SIMDS if slot_ms else None,
                      "residency_model_over_measured": (slot_ms / SIMDS / step_ms) if slot_ms else None,
                      "issue_utilisation": None,
                      "note": "residency_model_ms_per_step = sum over stages of (waves x duration alone) / (waves per SIMD its registers and LDS "
                              "allow) / 1024 SIMDs: the step time if the chip were exactly full of these waves, each living as long as its "
                              "launch does alone.  It OVER-estimates (a launch lasts as long as its slowest query; the mean workgroup is "
                              "shorter), so model / measured a little above 1 = the pipelined rate is what the wave slots allow; "
                              "ms_overlapped = a launch's duration while 12 streams overlap.  Resident wave-cycles and issue utilisation "
                              "from SQ counters: rocprofv3 passes in profiles/r4/ (not measured in this run)"}

    # Sensitivity of the headline to the data: the block-level bound and the lazy selection prune what the data lets them.
    # Same index shape and workload, intrinsic dimension 16 ... 128 and SURVEY 8d's isotropic recipe (rank 0, headline only).
    sensitivity = None
    if extras and is_headline and os.environ.get("RBQ_BENCH_SENSITIVITY", "1") != "0":
        try:
            del x
        except NameError:
            pass
        torch.cuda.empty_cache()
        rows = []
        hdr_src = built if built is not None else small
        for kind in ("mixture_id16", "mixture_id64", "mixture_id128"):
            mx = Mixture(torch, dev, a.dim, a.nlist, kind, False)
            xi = mx.draw(a.n, 20260105)
            ci, ai = kmeans_gpu(torch, xi, a.nlist, a.kmeans_iters, 20260103)
            idx2 = rq.IvfRabitqIndex.build_on_device(hdr_src.hdr_ptr, ci.cpu().numpy(), xi.data_ptr(), ai.to(torch.int32).contiguous().data_ptr(),
                                                     a.n, hdr_src.t_const, device=local)
            nb2 = min(NB, 8)
            qi = mx.draw(nb2 * a.batch, 20260102).contiguous().view(nb2, a.batch, a.dim)
            gti = exact_topk(torch, xi, qi.view(-1, a.dim), a.top_k, a.metric).cpu().numpy()
            del xi
            torch.cuda.empty_cache()
            dti, _, pi = run_measured(idx2, qi, a.nprobe, 48, 4, ns, gather=False)
            ri = recall_of(search_ids(idx2, qi, a.nprobe).reshape(-1, a.top_k), gti, a.top_k)
            po = pruned_object(pi, pi["counter_steps"])
            taps = lists_scanned(idx2, qi[0])
            rows.append({"dataset": kind, "intrinsic_dim": mx.idim, "recall_at_k": ri, "queries_per_s": a.batch * 48 / statistics.median(dti),
                         "block_skip_frac": po["block_skip_frac"], "lists_scanned_mean": taps, "nprobe": a.nprobe,
                         "bytes_requested_per_launch": po["bytes_requested_per_launch"]})
            idx2.close()
        rows.append({"dataset": a.dataset, "intrinsic_dim": INTRINSIC_DIM, "recall_at_k": recall, "queries_per_s": value / world,
                     "block_skip_frac": pruned["block_skip_frac"], "lists_scanned_mean": lists_scanned(idx, q_all[0]), "nprobe": a.nprobe,
                     "bytes_requested_per_launch": pruned["bytes_requested_per_launch"], "role": "headline"})
        sensitivity = {"by_dataset": sorted(rows, key=lambda r_: r_["intrinsic_dim"]),
                       "note": "x = mean_k + 0.35 z A / sqrt(id) + 0.1 eps, z in R^id; same N, d, nlist, nprobe, top_k, batch, streams; 48-step "
                               "regions; the isotropic recipe (intrinsic dimension = d) is in `datasets`"}

    what = f"N={a.n} d={a.dim}, nlist={a.nlist}, {a.bits}-bit, FhtKacRotator, {'L2' if a.metric == 0 else 'IP'}, nprobe={a.nprobe}, " \
           f"top_k={a.top_k}, batch={a.batch} per GPU"
    recall_ok = recall >= 0.95
    if is_headline:
        metric_name = "queries/sec at recall@10>=0.95, GIST-1M d=960, batch=1024"
        if not recall_ok:
            metric_name = f"queries/sec, GIST-1M-shaped d=960, batch=1024 (recall@10={recall:.3f} < 0.95: metric condition NOT met)"
    else:
        metric_name = f"queries/sec at recall@{a.top_k}={recall:.3f}, synthetic {a.dataset} {what}"
    out = {
        "metric": metric_name,
        "value": value,
        "unit": "queries/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": dt / a.steps * 1e3,
        "timed_regions": len(dts),  # value = the MEDIAN region; every region = exactly `steps` steps between barrier + synchronize
        "region_ms": [round(v * 1e3, 3) for v in dts],
        "per_rank_queries_per_s": per_rank,  # every rank's own median region (no max over ranks)
        "rccl_world_size": rccl_world,       # dist.get_world_size() of the nccl (= RCCL) group; null without one
        "preflight": preflight,              # N > 1: distinct devices == ranks was checked before anything was timed
        "host_issue_ms_per_step": prof["issue_s"] / a.steps * 1e3,  # host time to enqueue one step (launches + gather), rank 0
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "full": full,  # False: a plain run, the supplementary objects below are null
        # (the driver's record keeps `config` with its values but cuts strings at 128 characters and keeps only the NAMES of other
        # top-level objects: the short workload string and the numbers a reader of the one line needs live here)
        "config": {"workload": f"synthetic {a.dataset} N={a.n} d={a.dim} nlist={a.nlist} {a.bits}-bit {'L2' if a.metric == 0 else 'IP'} nprobe={a.nprobe} "
                               f"top_k={a.top_k} batch={a.batch}/GPU",
                   "workload_detail": f"synthetic GIST-1M-shaped fvecs ({a.dataset}) {what}",
                   "dataset_note": ("mixture_id32 is the FASTEST member of the intrinsic-dimension family {16, 32, 64, 128} (+5-12 % over the "
                                    "others: `sensitivity`); SURVEY 8d's isotropic recipe caps recall@10 at 0.93: `datasets`") if a.dataset == "mixture_id32" else None,
                   "parallelism": f"index replicated x{world}, queries sharded, RCCL all_gather of top-k",
                   "streams": ns, "distinct_query_batches": NB,
                   "scan_kernel": (regime or {}).get("scan_kernel"),
                   "host_call_queries_per_s": (host_call or {}).get("queries_per_s"),
                   "host_call_us_per_1024_query_call": ((host_call or {}).get("us_per_call") or {}).get("median"),
                   "latency_p50_us_1_query": ((latency or {}).get("1") or {}).get("p50_us") if isinstance(latency, dict) else None,
                   "latency_p50_us_64_queries": ((latency or {}).get("64") or {}).get("p50_us") if isinstance(latency, dict) else None,
                   "latency_p50_us_256_queries": ((latency or {}).get("256") or {}).get("p50_us") if isinstance(latency, dict) else None,
                   "value_is": "device-resident rate (queries and results in HBM); host_call_* = ONE rbq_search_batch call per step"},
        "recall_at_10" if a.top_k == 10 else f"recall_at_{a.top_k}": recall,
        "recall_ok": recall_ok,
        "recall_over_queries": NB * a.batch,
        "stage_ms": serial["stage_ms"] if serial else None,  # every stage alone on one stream
        "index_build_s": round(t_build, 1),
        "encoder": encoder,
        "rank_fallbacks": int(idx.rank_fallbacks()),
        "heap_restarts": int(idx.heap_restarts()),
        "tie_log": idx.tie_log_stats(),  # k_scan (host calls): tied queries that replayed their logged candidates instead of their lists
        "head_exact": dict(zip(("evaluations", "guard_trips"), idx.head_exact_stats())),
        "roofline": roofline,
        "pruned": pruned,
        "regime": regime,
        "sensitivity": sensitivity,
        "host_call": host_call,
        "pcie_inclusive": pcie,
        "latency": latency,
        "self_check": self_check,
        "datasets": datasets,
    }

    if full:
        mark("cpu baseline")
    if full and rank == 0 and world == 1 and not a.no_cpu and built is not None:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle  # CPU oracle: checker + reported baseline only
        qh0 = q_all[0].cpu().numpy()
        # threads: the box may hand this process fewer CPUs than it shows (cgroup quota / affinity): take the fastest of a
        # short sweep, so the baseline is the best the host cores given to this job can do
        avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        quota = None
        try:
            mx, per = open("/sys/fs/cgroup/cpu.max").read().split()
            if mx != "max":
                quota = max(1, int(round(int(mx) / int(per))))
        except (OSError, ValueError):
            pass
        omp_max = oracle.lib().ref_num_threads()
        cand = sorted({c for c in (quota, 8, 16, 32, avail, omp_max) if c and c <= max(avail, omp_max)})
        rc, oids, osc, ocnt, _ = oracle.search_batch(built, qh0, a.top_k, a.nprobe, nthreads=cand[0])  # warm-up pass + parity check
        sweep = {}
        for c in cand:  # informational: two passes per thread count, the better one
            best = 0.0
            for _ in range(2):
                t0 = time.perf_counter()
                oracle.search_batch(built, qh0, a.top_k, a.nprobe, nthreads=c)
                best = max(best, a.batch / max(time.perf_counter() - t0, 1e-6))
            sweep[c] = best
        # the FASTEST thread count of the sweep (pinning the baseline to the cgroup quota could only lower it; on this
        # pool the quota is 16 CPUs but 32 threads are often faster); the quota's own figure stays in thread_sweep_queries_per_s
        cores = max(sweep, key=sweep.get)
        pass_t = a.batch / sweep[cores]
        same = bool(np.array_equal(oids, ids_all[0]))
        same2 = None
        if NB > 1:  # a second batch of the rotation, so the check is not tied to batch 0
            rc2, oids2, _, _, _ = oracle.search_batch(built, q_all[NB - 1].cpu().numpy(), a.top_k, a.nprobe, nthreads=cores)
            same2 = bool(np.array_equal(oids2, ids_all[NB - 1]))
        reps = int(max(2, min(100, round(a.cpu_seconds * 0.6 / 3 / pass_t))))
        rates = []
        for _ in range(3):  # median of 3 timed repeats
            t0 = time.perf_counter()
            for _ in range(reps):
                oracle.search_batch(built, qh0, a.top_k, a.nprobe, nthreads=cores)
            rates.append(a.batch * reps / (time.perf_counter() - t0))
        # single thread, sequential queries: how the reference's own benches time it (examples/recall_qps_sweep.rs:127-138)
        ns1 = int(max(8, min(a.batch, 64)))
        t0 = time.perf_counter()
        oracle.search_batch(built, qh0[:ns1], a.top_k, a.nprobe, nthreads=1)
        one_t = max(time.perf_counter() - t0, 1e-3)
        ns1 = int(max(8, min(a.batch, round(ns1 * a.cpu_seconds * 0.4 / 3 / one_t))))
        r1 = []
        for _ in range(3):
            t0 = time.perf_counter()
            oracle.search_batch(built, qh0[:ns1], a.top_k, a.nprobe, nthreads=1)
            r1.append(ns1 / (time.perf_counter() - t0))
        out["cpu_baseline"] = {"value": statistics.median(rates), "unit": "queries/s", "cores": cores, "kind": "port",
                               "cpu_model": cpu_model(), "host_cpus": os.cpu_count(), "cpus_in_affinity_mask": avail, "cgroup_cpu_quota": quota,
                               "thread_sweep_queries_per_s": {str(k): v for k, v in sweep.items()},
                               "sample": f"query batch 0 ({a.batch} queries) on the same index, one query per thread (OpenMP static = "
                                         f"Rayon par_iter), threads = the fastest count of the sweep, median of 3 timed repeats of {reps} passes after warm-up passes",
                               "all_core_repeats": rates,
                               "single_thread": {"value": statistics.median(r1), "unit": "queries/s", "cores": 1, "repeats": r1,
                                                 "sample": f"first {ns1} queries of batch 0, sequential, median of 3"},
                               "ids_identical_to_gpu": same, "ids_identical_to_gpu_last_batch": same2,
                               "simd_level": int(oracle.lib().ref_simd_level()),
                               "note": "C restatement of the reference's fastest CPU variant, not the Rust binary (no toolchain)"}
        out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
    if rank == 0:
        print(json.dumps(out))
    if use_dist:
        dist.barrier()  # rank 0 has extra (supplementary) work behind it: nobody tears the group down early
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
