"""Rate of rbq_index_save_rbq1_stream (include/rbq_persist.h): an index trained on the GPU (IvfRabitqIndex.train, default
1M x 960, 7-bit, 4096 lists) saved to a discarding sink and to a file on local disk, then the file loaded back and searched
against the original handle.  Also the GPU CRC-32 (rbq_debug_crc32_device, the save path's kernels) against zlib.crc32 on
the host over the same bytes.  Prints one JSON line.  The per-kernel split comes from a separate run of this tool under
`rocprofv3 --kernel-trace --stats -- python tools/save_rate.py ...`."""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Discard:
    def __init__(self):
        self.n = 0

    def write(self, b):
        self.n += len(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--bits", type=int, default=7)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--dir", default=None, help="directory of the file written (default: the system temporary directory)")
    ap.add_argument("--seed", type=int, default=20261015)
    a = ap.parse_args()
    import torch
    import rabitq_rs_amd as rq
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    means = torch.randn(256, a.dim, device="cuda", generator=g)
    x = means[torch.randint(0, 256, (a.n,), device="cuda", generator=g)] + 0.35 * torch.randn(a.n, a.dim, device="cuda", generator=g)
    t0 = time.perf_counter()
    idx = rq.IvfRabitqIndex.train(x, a.nlist, a.bits, 0, 1, a.seed, False)
    t_train = time.perf_counter() - t0
    del x, means
    torch.cuda.empty_cache()
    out = {"n": a.n, "dim": a.dim, "bits": a.bits, "nlist": a.nlist, "train_s": t_train}

    sink = Discard()
    idx.save_to_writer(sink)  # warm-up (first-use costs of the kernels and pinned buffers)
    sink = Discard()
    t0 = time.perf_counter()
    idx.save_to_writer(sink)
    dt = time.perf_counter() - t0
    out["bytes"] = sink.n
    out["discard"] = {"s": dt, "GB_per_s": sink.n / dt / 1e9}

    fd, path = tempfile.mkstemp(suffix=".rbq", dir=a.dir)
    os.close(fd)
    try:
        t0 = time.perf_counter()
        idx.save_to_path(path)
        dt = time.perf_counter() - t0
        out["file"] = {"s": dt, "GB_per_s": sink.n / dt / 1e9}
        t0 = time.perf_counter()
        b = rq.IvfRabitqIndex.load_from_path(path)
        out["load_s"] = time.perf_counter() - t0
        with open(path, "rb") as f:
            data = f.read()
    finally:
        os.unlink(path)
    q = torch.randn((1024, a.dim), generator=torch.Generator().manual_seed(1)).numpy()
    ra = idx.batch_search_raw(q, rq.SearchParams(10, 64))
    rb = b.batch_search_raw(q, rq.SearchParams(10, 64))
    out["reloaded_search_identical"] = bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2]) and
                                            np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32)))
    b.close()

    # CRC-32 of the saved bytes: GPU kernels (device-resident copy) against zlib.crc32 on the host
    body = np.frombuffer(data, np.uint8)[8:-4]
    d = torch.from_numpy(body.copy()).cuda()
    rq.IvfRabitqIndex.debug_crc32_device(d.data_ptr(), body.size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    crc_gpu = rq.IvfRabitqIndex.debug_crc32_device(d.data_ptr(), body.size)
    dt_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    crc_host = zlib.crc32(memoryview(body)) & 0xFFFFFFFF
    dt_host = time.perf_counter() - t0
    stored = int.from_bytes(data[-4:], "little")
    out["crc"] = {"bytes": int(body.size), "gpu_s": dt_gpu, "gpu_GB_per_s": body.size / dt_gpu / 1e9,
                  "host_zlib_s": dt_host, "host_zlib_GB_per_s": body.size / dt_host / 1e9,
                  "equal": crc_gpu == crc_host == stored}
    idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
