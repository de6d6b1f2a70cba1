"""Faiss-style k-means, `run_kmeans_with_config` (reference src/kmeans.rs), on the GPU (rbq_kmeans_device, include/rbq_kmeans.h).

The arithmetic is pinned by the CPU restatement `builder.run_kmeans_with_config_cpu` (csrc/host/rbq_build.cpp), which the
device result equals bit for bit: centroids, assignments and objective."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi


@dataclass
class KMeansConfig:
    """`KMeansConfig` (src/kmeans.rs:13-37) with the crate's defaults."""
    niter: int = 25
    nredo: int = 1
    seed: int = 42
    spherical: bool = False
    max_points_per_centroid: int = 256
    decode_block_size: int = 32768


@dataclass
class KMeansResult:
    """`KMeansResult`: centroids [k][dim] f32, assignments [n] u32, objective (f64)."""
    centroids: np.ndarray
    assignments: np.ndarray
    objective: float


def _args(config):
    c = config if config is not None else KMeansConfig()
    return (int(c.niter), int(c.nredo), int(c.seed) & 0xFFFFFFFFFFFFFFFF, int(bool(c.spherical)),
            int(c.max_points_per_centroid), int(c.decode_block_size))


def validate(n, dim, k, config, finite):
    """The crate's checks (validate_inputs, src/kmeans.rs) with its messages, then what this project adds."""
    from . import RabitqError
    niter, nredo, _, _, mppc, dbs = _args(config)
    bad = None
    if n == 0:
        bad = "k-means requires non-empty data"
    elif k <= 0:
        bad = "k must be positive"
    elif niter <= 0:
        bad = "max_iter must be positive"
    elif k > n:
        bad = "k cannot exceed number of samples"
    elif nredo <= 0:
        bad = "nredo must be positive"
    elif dbs <= 0:
        bad = "decode_block_size must be positive"
    elif mppc < 0:
        bad = "max_points_per_centroid must not be negative"
    elif dim == 0:
        bad = "vectors must have at least one dimension"
    elif n >= 0xFFFFFFFF:
        bad = "k-means supports fewer than 2^32 - 1 vectors"
    elif not finite():
        bad = "k-means input must be finite"
    if bad:
        raise RabitqError(_abi.RBQ_INVALID_CONFIG, bad)


def first_draw(seed):
    """The first output of the project's Rng (splitmix64-seeded xoshiro256**, csrc/host/rbq_rng.h) seeded with `seed`:
    `rng.next_u64()` of IvfRabitqIndex::train's k-means seed."""
    m, z, st = (1 << 64) - 1, seed & ((1 << 64) - 1), []
    for _ in range(4):
        z = (z + 0x9E3779B97F4A7C15) & m
        x = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        st.append(x ^ (x >> 31))
    v = (st[1] * 5) & m
    return ((((v << 7) | (v >> 57)) & m) * 9) & m


def _run_device(x, k, config, device):
    """x: contiguous f32 CUDA tensor [n][dim] on `device` -> (centroids host, assignments int32 CUDA tensor, objective, stats)."""
    import torch
    from .index import _check, lib
    n, dim = int(x.shape[0]), int(x.shape[1])
    validate(n, dim, int(k), config, lambda: bool(torch.isfinite(x).all().item()))
    niter, nredo, seed, sph, mppc, dbs = _args(config)
    cent = np.empty((int(k), dim), np.float32)
    assign = torch.empty(n, dtype=torch.int32, device=x.device)
    obj = C.c_double()
    st = np.zeros(4, np.uint64)
    _check(lib().rbq_kmeans_device(C.c_void_p(x.data_ptr()), n, dim, int(k), niter, nredo, seed, sph, mppc, dbs, int(device),
                                   cent.ctypes.data, C.c_void_p(assign.data_ptr()), C.byref(obj), st.ctypes.data))
    return cent, assign, float(obj.value), dict(zip(_abi.KMEANS_STATS, (int(v) for v in st)))


def to_device(data, device):
    """`data` as a contiguous f32 CUDA tensor [n][dim] on `device` (numpy arrays are uploaded once)."""
    import torch
    from . import RabitqError
    dev = torch.device("cuda", int(device))
    if isinstance(data, torch.Tensor):
        x = data.to(device=dev, dtype=torch.float32).contiguous()
    else:
        x = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(dev)
    if x.dim() != 2:
        raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "data must be [n][dim]")
    return x


def debug_gemm_shortlist_front(centroids, rows, device=0, images=True):
    """TEST ONLY (rbq_debug_gemm_shortlist_front): what the shared front of the nearest-centroid paths computes for host
    `rows` [n][dim] against host `centroids` [k][dim].  A dict: dots [n][k], nx [n], nc [k] f32, ncmax (f32 scalar), and with
    `images` the split-bf16 planes row_hi, row_lo [n][Dp], cent_hi, cent_lo [k][Dp] u16 (Dp = dim rounded up to 32)."""
    from .index import _check, lib
    c = np.ascontiguousarray(centroids, dtype=np.float32)
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if c.ndim != 2 or x.ndim != 2 or x.shape[1] != c.shape[1]:
        from . import RabitqError
        raise RabitqError(_abi.RBQ_DIMENSION_MISMATCH, "centroids [k][dim] and rows [n][dim] must share dim")
    (k, dim), n = c.shape, x.shape[0]
    Dp =(dim + 31) // 32 * 32
    out = {"dots": np.empty((n, k), np.float32), "nx": np.empty(n, np.float32), "nc": np.empty(k, np.float32),
           "ncmax": np.empty(1, np.float32)}
    if images:
        out.update(row_hi=np.empty((n, Dp), np.uint16), row_lo=np.empty((n, Dp), np.uint16),
                   cent_hi=np.empty((k, Dp), np.uint16), cent_lo=np.empty((k, Dp), np.uint16))
    ptr = [out[f].ctypes.data if f in out else None for f in ("dots", "nx", "nc", "ncmax", "row_hi", "row_lo", "cent_hi", "cent_lo")]
    _check(lib().rbq_debug_gemm_shortlist_front(c.ctypes.data, k, dim, x.ctypes.data, n, int(device), *ptr))
    out["ncmax"] = out["ncmax"][0]
    return out


def run_kmeans_with_config(data, k, config=None, device=0, stats=None):
    """`run_kmeans_with_config` on `device`.  `data` [n][dim]: a numpy array (uploaded once) or a CUDA tensor (used in place
    when it is contiguous f32 on `device`).  Returns a KMeansResult with host arrays.  `stats`, when a dict, receives the run's
    counters: shortlist_fallbacks, empty_reseeded, rng_draws, max_shortlist."""
    cent, assign, obj, st = _run_device(to_device(data, device), k, config, device)
    if stats is not None:
        stats.update(st)
    return KMeansResult(cent, assign.cpu().numpy().view(np.uint32), obj)
