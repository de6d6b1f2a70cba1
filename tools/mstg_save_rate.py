"""Rate of the `.mstg` writer and loader (include/rbq_mstg_persist.h): an MSTG index built on the GPU
(default 1 M x 960, 7 bits, centroids from a subsample) saved to a discarding sink and to a file, the file loaded back and
searched against the original handle, and — the comparison — the same bytes assembled on the HOST in NumPy from the handle's
debug_copy_index arrays (a slice of the lists, scaled by bytes).  Against section 12's RBQ1 figures compare GB/s.  Runs under
a time limit of its own (--limit seconds: SIGALRM ends the process) and writes one JSON object to --out.  The per-kernel split
comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/mstg_save_rate.py ...`."""
import argparse
import json
import os
import signal
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Discard:
    def __init__(self):
        self.n = 0

    def write(self, b):
        self.n += len(b)


def host_list_bytes(c, cent, n, gb0, arrays, D, ex_bits, t_const):
    """The bytes of posting list c (length prefix included) from the device-layout arrays, on the host."""
    Dc = (D + 63) // 64 * 64
    G16, nb = Dc >> 7, (n + 31) // 32
    E = D // 16 * {0: 2, 2: 4, 6: 12}[ex_bits]
    R = 73 + 2 * D + D // 8 + E
    tb, t = (ex_bits + 1, t_const) if n else (7, None)
    head = struct.pack("<IQ", c, D) + cent.tobytes() + struct.pack("<IQ", n, tb) + (b"\0" if t is None else b"\1" + np.float32(t).tobytes())
    head += struct.pack("<Q", n)
    if n == 0:
        return struct.pack("<Q", len(head)) + head
    blk = arrays["blocks"].reshape(-1, Dc * 4 + 384)[gb0:gb0 + nb]
    code = np.zeros((nb, 32, Dc // 8), np.uint8)  # packed sign bytes per vector
    code[:, :, :G16 * 16] = blk[:, :G16 * 512].reshape(nb, G16, 32, 16).transpose(0, 2, 1, 3).reshape(nb, 32, G16 * 16)
    if Dc & 64:
        code[:, :, G16 * 16:] = blk[:, G16 * 512:G16 * 512 + 256].reshape(nb, 32, 8)
    binp = code.reshape(nb * 32, -1)[:n, :D // 8]
    bits = np.unpackbits(binp, axis=1, bitorder="big").astype(np.uint16)
    fac = blk[:, Dc * 4:].copy().view(np.float32).reshape(nb, 3, 32)
    sl = slice(gb0 * 32, gb0 * 32 + n)
    ex = np.zeros((n, D), np.uint16)
    if ex_bits:
        cpu = 128 // ex_bits
        w4 = (D // 16 + cpu - 1) // cpu
        u = arrays["ex"].reshape(-1, w4, 16, 16)[sl]                                    # [n][unit][lane][16 B]
        b = np.unpackbits(u, axis=3, bitorder="little")[..., :cpu * ex_bits].reshape(n, w4, 16, cpu, ex_bits)
        codes = (b.astype(np.uint16) << np.arange(ex_bits, dtype=np.uint16)).sum(axis=4)  # [n][unit][lane][k]: dim 16 (unit cpu + k) + lane
        ex = codes.transpose(0, 1, 3, 2).reshape(n, w4 * cpu * 16)[:, :D].astype(np.uint16)
    g = ex.reshape(n, D // 16, 16)
    two = lambda x: sum((x[:, :, 4 * q:4 * q + 4] & 3) << (2 * q) for q in range(4))  # noqa: E731
    exp = (np.zeros((n, E), np.uint8) if ex_bits == 0 else two(g).astype(np.uint8).reshape(n, -1) if ex_bits == 2 else
           np.concatenate([(g[:, :, :8] & 15) | ((g[:, :, 8:] & 15) << 4), two(g >> 4)], axis=2).astype(np.uint8).reshape(n, -1))
    rec = np.empty((n, R), np.uint8)
    o = 0
    zero = np.zeros(n, np.float32)
    f32 = lambda name: arrays[name][sl] if name in arrays else zero  # noqa: E731
    u64 = lambda v: np.full(n, v, "<u8")  # noqa: E731
    for a in (arrays["ids"][sl], u64(D), (ex + (bits << ex_bits)).astype("<u2"), u64(D // 8), binp, u64(E), exp,
              np.full(n, ex_bits, np.uint8), u64(D), f32("delta"), f32("vl"), fac[:, 0].reshape(-1)[:n], fac[:, 1].reshape(-1)[:n],
              fac[:, 2].reshape(-1)[:n], f32("rnorm"), f32("fadd_ex"), f32("fres_ex")):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(n, -1)
        rec[:, o:o + a.shape[1]] = a
        o += a.shape[1]
    assert o == R
    body = head + rec.tobytes()
    return struct.pack("<Q", len(body)) + body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--lists", type=int, default=16384)
    ap.add_argument("--host-lists", type=int, default=256, help="lists assembled on the host (their time is scaled by bytes)")
    ap.add_argument("--dir", default=None, help="directory of the file written (default: the system temporary directory)")
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--limit", type=int, default=900, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mstg_save_rate.json"))
    a = ap.parse_args()
    signal.alarm(a.limit)
    import torch
    import rabitq_rs_amd as rq
    from rabitq_rs_amd import mstg
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    means = torch.randn(256, a.dim, device="cuda", generator=g)
    x = means[torch.randint(0, 256, (a.n,), device="cuda", generator=g)] + 0.35 * torch.randn(a.n, a.dim, device="cuda", generator=g)
    cent = x[torch.randperm(a.n, device="cuda", generator=g)[:a.lists]].cpu().numpy()
    t0 = time.perf_counter()
    idx = rq.build_postings_on_device(x, cent, a.bits, 0, faster_config=True)
    torch.cuda.synchronize()
    out = {"n": a.n, "dim": a.dim, "bits": a.bits, "lists": a.lists, "pairs": len(idx), "build_s": time.perf_counter() - t0,
           "device_bytes": mstg.memory_usage(idx)}
    cfg = dict(max_posting_size=5000, branching_factor=10, balance_weight=1.0, closure_epsilon=0.15, max_replicas=8, rabitq_bits=a.bits,
               faster_config=True, metric=0, hnsw_m=32, hnsw_ef_construction=200, centroid_precision=1, default_ef_search=150,
               pruning_epsilon=0.6)
    mstg.save_mstg(idx, cfg, Discard())  # warm-up (first-use costs of the kernels and pinned buffers)
    sink = Discard()
    t0 = time.perf_counter()
    mstg.save_mstg(idx, cfg, sink)
    dt = time.perf_counter() - t0
    out["bytes"] = sink.n
    out["discard"] = {"s": dt, "GB_per_s": sink.n / dt / 1e9}
    fd, path = tempfile.mkstemp(suffix=".mstg", dir=a.dir)
    os.close(fd)
    try:
        t0 = time.perf_counter()
        mstg.save_mstg(idx, cfg, path)
        dt = time.perf_counter() - t0
        out["file"] = {"s": dt, "GB_per_s": sink.n / dt / 1e9}
        t0 = time.perf_counter()
        back, _ = mstg.load_mstg(path)
        out["load"] = {"s": time.perf_counter() - t0, "GB_per_s": sink.n / (time.perf_counter() - t0) / 1e9}
        q = x[:1024].cpu().numpy()
        r0, r1 = mstg.mstg_search(idx, q, 10), mstg.mstg_search(back, q, 10)
        out["reload_identical"] = all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(r0, r1))
        back.close()
        # host leg: the first --host-lists lists from the device-layout arrays, checked against the file
        k, D, ex = idx.cluster_count(), a.dim, a.bits - 1
        ln = idx.debug_copy_index("list_n", np.empty(k, np.uint32)).astype(np.int64)
        gb0 = idx.debug_copy_index("list_gb0", np.empty(k, np.uint32)).astype(np.int64)
        nb = int(((ln + 31) // 32).sum())
        Dc = (D + 63) // 64 * 64
        cpu = 128 // ex if ex else 1
        w4 = ((D // 16 + cpu - 1) // cpu) if ex else 0
        t0 = time.perf_counter()
        arrays = {"blocks": idx.debug_copy_index("blocks", np.empty(nb * (Dc * 4 + 384), np.uint8)),
                  "ids": idx.debug_copy_index("ids", np.empty(nb * 32, np.uint64))}
        for name in ("delta", "vl", "rnorm") + (("fadd_ex", "fres_ex") if ex else ()):
            arrays[name] = idx.debug_copy_index(name, np.empty(nb * 32, np.float32))
        if ex:
            arrays["ex"] = idx.debug_copy_index("ex", np.empty(nb * 32 * w4 * 256, np.uint8))
        t_copy = time.perf_counter() - t0
        centroids = idx.debug_copy_index("centroids", np.empty((k, D), np.float32))
        from rabitq_rs_amd import builder
        small = builder.train_with_clusters(centroids[:1], centroids[:1], np.zeros(1, np.uint32), a.bits, 0, rq.RotatorType.NoRotation, 42, True)
        t_const = small.t_const if ex else None
        small.close()
        hl = min(a.host_lists, k)
        t0 = time.perf_counter()
        host = b"".join(host_list_bytes(c, centroids[c], int(ln[c]), int(gb0[c]), arrays, D, ex, t_const) for c in range(hl))
        t_host = time.perf_counter() - t0
        first = 8 + 8 + 77 + 8 + 4 * k + 8
        with open(path, "rb") as f:
            f.seek(first)
            same = f.read(len(host)) == host
        out["host"] = {"lists": hl, "bytes": len(host), "s": t_host, "GB_per_s": len(host) / t_host / 1e9, "identical": same,
                       "copy_arrays_s": t_copy, "scaled_to_all_s": t_copy + t_host * (sink.n - first) / max(len(host), 1)}
    finally:
        os.unlink(path)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
