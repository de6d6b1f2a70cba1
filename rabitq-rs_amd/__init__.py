"""rabitq_rs_amd — MI355X-native IVF+RaBitQ candidate-scan engine (host-side Python mirror).

Mirrors the reference's public query API for this path:
  SearchParams{top_k,nprobe}   src/ivf.rs:23-26,137-141
  SearchResult{id,score}       src/ivf.rs:143-148
  RabitqError                  src/lib.rs:39-57
  Metric                       src/lib.rs:18-37
  IvfRabitqIndex.search / search_filtered / batch_search / len / cluster_count
                               src/ivf.rs:1705-1752,1218-1230
  BruteForceRabitqIndex        src/brute_force.rs (bruteforce.py)
  KMeansConfig / run_kmeans_with_config, IvfRabitqIndex.train
                               src/kmeans.rs, src/ivf.rs:950-1021 (kmeans.py)
  closure_assign / build_postings_on_device: MstgIndex::build steps 2 and 3
                               src/mstg/closure.rs, src/mstg/index.rs:40-110 (mstg.py)
  mstg_search / select_lists_cpu / MstgSearchParams: MstgIndex::search and batch_search
                               src/mstg/index.rs:149-213,340-362 (mstg.py)
  mstg_search(..., refine_pool=n): opt-in, no crate counterpart: the binary candidates re-scored with the ex codes
                               (the refinement of src/ivf.rs:2086-2099), every id once (mstg.py)
  mstg_search(..., refine_pool=n, exact=True), MstgIndex.set_rerank_vectors: opt-in, no crate counterpart: the pool scored
                               exactly against attached raw vectors (l2_distance_sqr / dot of src/math.rs), every id once (mstg.py)
  hierarchical_cluster / hierarchical_cluster_cpu / MstgIndex: HierarchicalClustering::cluster, PyMstgIndex
                               src/mstg/clustering.rs, src/python_bindings.rs (mstg.py)
  save_mstg / load_mstg, MstgIndex.save / load / get_memory_usage: MstgIndex::save_main_index / load_main_index
                               src/mstg/io.rs:129-245 (mstg.py)
  append_postings / remove_postings, MstgIndex.add / remove_ids / id_bound: no crate counterpart (its MstgIndex is immutable):
                               FAISS-style add and remove_ids on posting-list handles, equal to a rebuild (mstg.py)
All compute goes through the C ABI of include/rbq.h (csrc/librbq.so, hand-written HIP for
gfx950). There is no CPU fallback: if the HIP library is missing or no GPU is present the
calls raise.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import (METRIC_IP, METRIC_L2, ROTATOR_FHT_KAC, ROTATOR_MATRIX, ROTATOR_NONE, RBQ_OK)


class Metric:
    L2 = METRIC_L2
    InnerProduct = METRIC_IP


class RotatorType:
    MatrixRotator = ROTATOR_MATRIX
    FhtKacRotator = ROTATOR_FHT_KAC
    NoRotation = ROTATOR_NONE  # MSTG posting lists (quantised in the raw space)


_ERR_NAMES = {
    _abi.RBQ_DIMENSION_MISMATCH: "DimensionMismatch",
    _abi.RBQ_INVALID_CONFIG: "InvalidConfig",
    _abi.RBQ_EMPTY_INDEX: "EmptyIndex",
    _abi.RBQ_IO: "Io",
    _abi.RBQ_INVALID_PERSISTENCE: "InvalidPersistence",
    _abi.RBQ_DEVICE: "Device",
}


class RabitqError(Exception):
    """`RabitqError` (src/lib.rs:39-57) + Device for HIP failures."""

    def __init__(self, code, detail=""):
        self.code = code
        self.kind = _ERR_NAMES.get(code, f"Unknown({code})")
        self.detail = detail
        super().__init__(f"{self.kind}: {detail}" if detail else self.kind)


@dataclass(frozen=True)
class SearchParams:
    top_k: int
    nprobe: int


@dataclass(frozen=True)
class SearchResult:
    id: int
    score: float


from .index import IvfRabitqIndex, StreamBuilder  # noqa: E402
from . import builder  # noqa: E402,F401
from .bruteforce import BruteForceRabitqIndex, BruteForceSearchParams, BruteForceSearchResult  # noqa: E402
from .kmeans import KMeansConfig, KMeansResult, run_kmeans_with_config  # noqa: E402
from .mstg import (MstgIndex, MstgSearchParams, append_postings, build_postings_on_device, closure_assign,  # noqa: E402
                   closure_assign_cpu, hierarchical_cluster, hierarchical_cluster_cpu, load_mstg, mstg_search, remove_postings,
                   save_mstg, select_lists_cpu)

__all__ = ["Metric", "RotatorType", "RabitqError", "SearchParams", "SearchResult", "IvfRabitqIndex",
           "StreamBuilder", "builder", "BruteForceRabitqIndex", "BruteForceSearchParams", "BruteForceSearchResult",
           "KMeansConfig", "KMeansResult", "run_kmeans_with_config", "closure_assign", "closure_assign_cpu",
           "build_postings_on_device", "MstgSearchParams", "mstg_search", "select_lists_cpu", "hierarchical_cluster",
           "hierarchical_cluster_cpu", "MstgIndex", "save_mstg", "load_mstg", "append_postings", "remove_postings"]
