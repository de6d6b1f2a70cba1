"""Cost of shrinking a device-resident index with rbq_index_remove_ids against the only thing the library offered before it: a
rebuild of the rows that stay with rbq_index_build_device_ex, which needs every raw row resident.

Set-up: a Gaussian mixture of the shape of bench.py's headline set (1 M x 960, 4096 lists, 7-bit, constant rescale), resident on
the GPU, encoded into an index of --n rows; --add (100 k) further device-resident rows appended with rbq_index_append.  Then
  1 %, 10 % and 50 % of the --n ids, chosen at random, are removed from the --n index       (random_1 / random_10 / random_50)
  the --add most recently appended ids are removed from the grown index                     (recent)
each against a rebuild of the kept rows (gathered on the device beforehand; the gather is not timed).  Wall seconds of one call
after a warm-up call of the same kind, host overheads included; the set is a device-resident u64 array.  The gather kernel
moves the old index into the shrunk geometry; its device time comes from the library (rbq_debug_remove_gather_ns), its bytes
from the geometry, as the bytes the kernel REQUESTS: every survivor's share of its old block is read (a 32nd of the record,
ids, ex codes, ex factors, delta, vl: the lanes that go are not loaded, though the 128-byte lines around them may be fetched),
every block of the new index is written whole, and the slot map is read.  The rate stands beside the append's carry (4.4 TB/s
recorded) and the ~6.3 TB/s a copy achieves on an MI355X.  Prints one JSON line; --out writes it to a file
(profiles/remove_rate_1m_d960.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--add", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    from encode_rate import make_data
    from rabitq_rs_amd.index import _check, lib
    x, cent, assign = make_data(torch, a.n + a.add, a.dim, a.nlist, a.seed)
    cent_h = cent.cpu().numpy()
    small = rq.builder.train_with_clusters(x[:a.nlist].cpu().numpy(), cent_h, np.arange(a.nlist, dtype=np.uint32), a.bits, 0, 1, a.seed, True)
    t_const = small.t_const
    D = (a.dim + 63) // 64 * 64
    ex = a.bits - 1
    cpu_u = 128 // ex if ex else 1
    exd = ((D // 16 + cpu_u - 1) // cpu_u) * 256 if ex else 0
    per_block = D * 4 + 384 + 256 + 32 * exd + (4 if ex else 2) * 128

    def build(rows, asg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = rq.IvfRabitqIndex.build_on_device(small.hdr_ptr, cent_h, rows.data_ptr(), asg.data_ptr(), rows.shape[0], t_const, rescale="const")
        return idx, time.perf_counter() - t0

    def remove(base, ids):
        h, removed = C.c_void_p(), C.c_uint64()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _check(lib().rbq_index_remove_ids(base._h, C.c_void_p(ids.data_ptr()), ids.numel(), 1, None, C.byref(removed), C.byref(h)))
        dt = time.perf_counter() - t0
        return rq.IvfRabitqIndex(h), dt, int(lib().rbq_debug_remove_gather_ns()), int(removed.value)

    def case(base, n_base, ids):
        """one removal after a warm-up of the same kind, and the rebuild of the kept rows"""
        warm, _, _, _ = remove(base, ids)
        warm.close()
        ln_old = base.debug_copy_index("list_n", np.empty(a.nlist, np.uint32)).astype(np.int64)
        shrunk, dt, ns, removed = remove(base, ids)
        assert removed == ids.numel() and len(shrunk) == n_base - removed
        ln_new = shrunk.debug_copy_index("list_n", np.empty(a.nlist, np.uint32)).astype(np.int64)
        shrunk.close()
        keep = torch.ones(n_base, dtype=torch.bool, device="cuda")
        keep[ids] = False
        rows, asg = x[:n_base][keep].contiguous(), assign[:n_base][keep].contiguous()
        del keep
        re, t_rebuild = build(rows, asg)
        re.close()
        del rows, asg
        torch.cuda.empty_cache()
        nb_old, nb_new = int(((ln_old + 31) // 32).sum()), int(((ln_new + 31) // 32).sum())
        read = (n_base - removed) * (per_block // 32) + nb_new * 128
        moved = read + nb_new * per_block
        return {"removed": removed, "remove_s": round(dt, 4), "rebuild_kept_rows_s": round(t_rebuild, 4),
                "rebuild_over_remove": round(t_rebuild / dt, 2),
                "gather": {"old_blocks": nb_old, "blocks_written": nb_new, "bytes_per_block": per_block, "bytes_read": read, "bytes_moved": moved,
                           "kernel_s": round(ns * 1e-9, 6), "tb_per_s": round(moved / max(ns, 1) * 1e-3, 3)}}

    base, _ = build(x[:a.n], assign[:a.n].contiguous())  # (also the warm-up of the encoder's code objects)
    g = torch.Generator(device="cpu").manual_seed(a.seed)
    perm = torch.randperm(a.n, generator=g)
    rec = {"tool": "remove_rate", "n": a.n, "add": a.add, "dim": a.dim, "bits": a.bits, "nlist": a.nlist,
           "carry_tb_per_s_recorded": 4.4, "achievable_tb_per_s": 6.3}
    for pct in (1, 10, 50):
        ids = perm[:a.n * pct // 100].to(torch.int64).cuda().contiguous()
        rec["random_%d" % pct] = case(base, a.n, ids)
    h = C.c_void_p()
    _check(lib().rbq_index_append(base._h, C.c_void_p(x[a.n:].data_ptr()), C.c_void_p(assign[a.n:].contiguous().data_ptr()), a.add, a.n, 0,
                                  t_const, 0, 1, None, None, C.byref(h)))
    base.close()
    grown = rq.IvfRabitqIndex(h)
    rec["recent"] = case(grown, a.n + a.add, torch.arange(a.n, a.n + a.add, dtype=torch.int64, device="cuda"))
    grown.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
