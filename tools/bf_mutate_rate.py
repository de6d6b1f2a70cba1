"""Cost of growing, shrinking and reading back a device-resident brute-force index (rbq_bf_append, rbq_bf_remove_ids,
rbq_bf_fetch_embeddings*) against the only thing the library offered before them: training again with rbq_bf_train_device over
the rows the index then holds, which needs every raw row resident.

Set-up: the shape of profiles/bf_train_rate_200k_d1024.json: --n (200 000) x --dim (1024) Gaussian rows resident on the GPU,
7-bit, FHT-Kac, L2, both rescale modes.  Per mode:
  append        --add (20 000) further device-resident rows appended              against training over all --n + --add rows
  remove_P      P = 1, 10, 50 per cent of the ids at random (a device u64 array)  against training over the kept rows (gathered
                                                                                  on the device beforehand; not timed)
  fetch         --fetch (10 000) random ids through the host entry (pageable buffers) and through the device entry
Every timing is the wall time of one call between two device synchronisations, host overheads included; an operation and its
baseline alternate, --repeats times after one warm-up of each, and the median, minimum and maximum are recorded.  The gather
kernel's device time comes from the library (rbq_bf_debug_remove_gather_ns), its bytes from the shapes, as the bytes the kernel
REQUESTS: every survivor's sign code, ex code and eight factors are read and written once, and its map entry is read.  The
append's carry copies are timed the same way (rbq_bf_debug_append_carry_ns): the old arrays read and written once.  A copy
achieves about 6.3 TB/s of HBM traffic on an MI355X.  Needs a GPU: there is no CPU path.  Prints one JSON line; --out writes it
to a file (profiles/bf_mutate_rate.json)."""
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


def stats(ts):
    return {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--add", type=int, default=20_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--fetch", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    from rabitq_rs_amd import bruteforce as bfm
    from rabitq_rs_amd.index import _check
    if not torch.cuda.is_available():
        sys.exit("bf_mutate_rate needs a GPU: nothing is measured without one")
    lib = bfm.lib()
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    x = torch.randn((a.n + a.add, a.dim), generator=g, device="cuda", dtype=torch.float32)
    row0 = x[:1].cpu().numpy()
    perm = torch.randperm(a.n, generator=torch.Generator(device="cpu").manual_seed(a.seed))
    fetch_ids = np.random.default_rng(a.seed).integers(0, a.n, a.fetch).astype(np.uint64)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def versus(op, base):
        """op() and base() return a handle: alternated after one warm-up of each; the last handle of op() is returned open"""
        for fn in (op, base):
            lib.rbq_bf_destroy(fn())
        t_op, t_base, last = [], [], None
        for _ in range(a.repeats):
            if last:
                lib.rbq_bf_destroy(last)
            last, dt = timed(op)
            t_op.append(dt)
            h, dt = timed(base)
            t_base.append(dt)
            lib.rbq_bf_destroy(h)
        return last, t_op, t_base

    rec = {"tool": "bf_mutate_rate", "n": a.n, "add": a.add, "dim": a.dim, "bits": a.bits, "rotator": "fht_kac", "metric": "l2",
           "fetch": a.fetch, "repeats": a.repeats, "achievable_tb_per_s": 6.3, "modes": {}}
    for mode, faster in (("const", True), ("optimal", False)):
        small = rq.builder.train_bruteforce(row0, a.bits, 0, 1, a.seed, faster)
        hdr, t_const = C.cast(small.hdr_ptr, C.c_void_p), small.t_const
        rescale = rq._abi.RESCALE_CONST if faster else rq._abi.RESCALE_OPTIMAL
        D = int(small.header.padded_dim)
        row_bytes = D // 8 + D * (a.bits - 1) // 8 + 32

        def train(rows):
            h = C.c_void_p()
            _check(lib.rbq_bf_train_device(hdr, C.c_void_p(rows.data_ptr()), rows.shape[0], rescale, t_const, 0, -1, C.byref(h)))
            return h

        base = train(x[:a.n])
        out = {}

        def append():
            h = C.c_void_p()
            _check(lib.rbq_bf_append(base, C.c_void_p(x[a.n:].data_ptr()), a.add, rescale, t_const, 0, C.byref(h)))
            return h

        grown, t_op, t_base = versus(append, lambda: train(x))
        carry_ns = int(lib.rbq_bf_debug_append_carry_ns())
        assert lib.rbq_bf_len(grown) == a.n + a.add
        lib.rbq_bf_destroy(grown)
        out["append"] = {"append": stats(t_op), "train_all_rows": stats(t_base),
                         "train_over_append": round(statistics.median(t_base) / statistics.median(t_op), 2),
                         "carry": {"bytes_moved": 2 * a.n * row_bytes, "copies_s": round(carry_ns * 1e-9, 6),
                                   "tb_per_s": round(2 * a.n * row_bytes / max(carry_ns, 1) * 1e-3, 3)}}
        for pct in (1, 10, 50):
            ids = perm[:a.n * pct // 100].to(torch.int64).cuda().contiguous()
            keep = torch.ones(a.n, dtype=torch.bool, device="cuda")
            keep[ids] = False
            kept_rows = x[:a.n][keep].contiguous()
            del keep

            def remove():
                h, removed = C.c_void_p(), C.c_uint64()
                _check(lib.rbq_bf_remove_ids(base, C.c_void_p(ids.data_ptr()), ids.numel(), C.byref(removed), C.byref(h)))
                assert removed.value == ids.numel()
                return h

            shrunk, t_op, t_base = versus(remove, lambda: train(kept_rows))
            ns = int(lib.rbq_bf_debug_remove_gather_ns())
            kept = int(lib.rbq_bf_len(shrunk))
            assert kept == a.n - ids.numel()
            lib.rbq_bf_destroy(shrunk)
            moved = kept * (2 * row_bytes + 4)
            out["remove_%d" % pct] = {"removed": int(ids.numel()), "remove": stats(t_op), "train_kept_rows": stats(t_base),
                                      "train_over_remove": round(statistics.median(t_base) / statistics.median(t_op), 2),
                                      "gather": {"bytes_per_row": row_bytes, "bytes_moved": moved, "kernel_s": round(ns * 1e-9, 6),
                                                 "tb_per_s": round(moved / max(ns, 1) * 1e-3, 3)}}
            del kept_rows, ids
            torch.cuda.empty_cache()
        vec, found = np.empty((a.fetch, a.dim), np.float32), np.empty(a.fetch, np.uint8)
        d_ids = torch.from_numpy(fetch_ids.view(np.int64)).cuda()
        d_out = torch.empty((a.fetch, a.dim), dtype=torch.float32, device="cuda")
        d_found = torch.empty(a.fetch, dtype=torch.uint8, device="cuda")
        host = lambda: _check(lib.rbq_bf_fetch_embeddings(base, fetch_ids.ctypes.data, a.fetch, vec.ctypes.data, found.ctypes.data))  # noqa: E731
        dev = lambda: _check(lib.rbq_bf_fetch_embeddings_device(base, d_ids.data_ptr(), a.fetch, d_out.data_ptr(), d_found.data_ptr(), None))  # noqa: E731
        host(), dev()
        t_host, t_dev = [], []
        for _ in range(a.repeats):
            t_host.append(timed(host)[1])
            t_dev.append(timed(dev)[1])
        assert found.all() and np.array_equal(d_out.cpu().numpy().view(np.uint32), vec.view(np.uint32))
        out["fetch"] = {"host_entry": dict(stats(t_host), ids_per_s=round(a.fetch / statistics.median(t_host), 1)),
                        "device_entry": dict(stats(t_dev), ids_per_s=round(a.fetch / statistics.median(t_dev), 1))}
        lib.rbq_bf_destroy(base)
        small.close()
        rec["modes"][mode] = out
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
