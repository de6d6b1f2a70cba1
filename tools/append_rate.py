"""Cost of growing a device-resident index with rbq_index_append against the only thing the library offered before it: a
rebuild of every row with rbq_index_build_device_ex.

Set-up: a Gaussian mixture of the shape of bench.py's headline set (1 M x 960, 4096 lists, 7-bit, constant rescale), resident on
the GPU, encoded into an index; then --add (100 k) further device-resident rows are
  appended with their lists given          (append_assign_s)
  appended with assign = NULL              (append_nearest_s: rotation, nearest-centroid assignment, then the same)
  and all n + add rows are rebuilt at once (rebuild_s; the lists of the new rows are the nearest-centroid ones).
Wall seconds of each call, host overheads included.  The carry kernel moves the old index into the grown geometry; its device
time comes from the library (rbq_debug_append_carry_ns), its bytes from the geometry: every block of the old index is read and
every block of the new one written (record, ids, ex codes, ex factors, delta, vl), and both count.  The rate stands beside the
~6.3 TB/s a copy achieves on an MI355X.  Prints one JSON line; --out writes it to a file (profiles/append_rate_1m_d960.json)."""
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

    def build(n, asg):
        return rq.IvfRabitqIndex.build_on_device(small.hdr_ptr, cent_h, x.data_ptr(), asg.data_ptr(), n, t_const, rescale="const")

    def append(base, asg, out_assign=None):
        h = C.c_void_p()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _check(lib().rbq_index_append(base._h, C.c_void_p(x[a.n:].data_ptr()), None if asg is None else C.c_void_p(asg.data_ptr()), a.add,
                                      a.n, 0, t_const, 0, 1, None, None if out_assign is None else C.c_void_p(out_assign.data_ptr()),
                                      C.byref(h)))
        dt = time.perf_counter() - t0
        return rq.IvfRabitqIndex(h), dt, int(lib().rbq_debug_append_carry_ns())

    base = build(a.n, assign)  # (also the warm-up of the encoder's code objects)
    base.id_bound()
    warm, _, _ = append(base, assign[a.n:].contiguous())
    warm.close()
    grown, t_assign, carry_ns = append(base, assign[a.n:].contiguous())
    ln_old = base.debug_copy_index("list_n", np.empty(a.nlist, np.uint32)).astype(np.int64)
    ln_new = grown.debug_copy_index("list_n", np.empty(a.nlist, np.uint32)).astype(np.int64)
    grown.close()
    near = torch.empty(a.add, dtype=torch.int32, device="cuda")
    warm, _, _ = append(base, None, near)
    warm.close()
    grown, t_near, _ = append(base, None, near)
    assert len(grown) == a.n + a.add
    grown.close()
    base.close()
    all_assign = torch.cat([assign[:a.n], near]).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    full = build(a.n + a.add, all_assign)
    t_rebuild = time.perf_counter() - t0
    full.close()

    D = (a.dim + 63) // 64 * 64
    ex = a.bits - 1
    cpu_u = 128 // ex if ex else 1
    exd = ((D // 16 + cpu_u - 1) // cpu_u) * 256 if ex else 0
    per_block = D * 4 + 384 + 256 + 32 * exd + (4 if ex else 2) * 128
    nb_old, nb_new = int(((ln_old + 31) // 32).sum()), int(((ln_new + 31) // 32).sum())
    moved = (nb_old + nb_new) * per_block
    rec = {"tool": "append_rate", "n": a.n, "add": a.add, "dim": a.dim, "bits": a.bits, "nlist": a.nlist,
           "append_assign_s": round(t_assign, 4), "append_nearest_s": round(t_near, 4), "rebuild_s": round(t_rebuild, 4),
           "rebuild_over_append_assign": round(t_rebuild / t_assign, 2), "rebuild_over_append_nearest": round(t_rebuild / t_near, 2),
           "carry": {"blocks_read": nb_old, "blocks_written": nb_new, "bytes_per_block": per_block, "bytes_moved": moved,
                     "kernel_s": round(carry_ns * 1e-9, 6), "tb_per_s": round(moved / max(carry_ns, 1) * 1e-3, 3),
                     "achievable_tb_per_s": 6.3}}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
