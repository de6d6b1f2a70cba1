"""Everything the three routes of probe selection hand to the scan, held together on one input.

k_select (the all-pairs canonical ranking of exact_rank = 1), k_select_mfma's approximate path (the default) and k_select_mfma's
canonical branch (force_rank_fallback = 1, which a query also takes by itself when its approximate scores are not finite) share their
steps as device functions (select_common.hpp: the radix select of the nprobe-th key, the bitonic network, the per-probe constants, the
block stream and its bound) and must agree bit for bit: the scan trusts lbmin, and the tests of exact_rank compare with the default.
With lazy_select = 0 every route streams all nprobe lists, so for one index and one batch the search runs through
  (a) exact_rank = 1            k_rank_scores + k_select
  (b) defaults                  the ranking GEMM + k_select_mfma, and rank_fallbacks() does not move
  (c) force_rank_fallback = 1   the ranking GEMM + k_select_mfma's canonical branch, and the counter moves by the number of queries
and the route is read from stage_resources() (what the rank stage multiplies, and a select kernel of other resources for (a)).
Compared bit for bit: the workspace copies probe [nq][nprobe][4] (g_add, g_err, dotqc, list id), nstream, nvec and the stream entries
wl[q][:nstream[q]] (block, rank << 6 | nvalid, lbmin, 0), and the ids, scores and counts of the search.
Shapes, the smallest that reach each piece:
  base       2000 vectors, 16 lists, 7 bits, 5 queries (one an exact copy of a centroid), both metrics, dims 64 and 100 (padded to 128),
             nprobe 4 and nprobe 16 = n_lists (no radix select, prefix ~0), top_k 10
  ties       two centroids are exact duplicates (two keys differ in the id word only: the radix select's last four passes, the sort's
             tie order) and one probed list has no vectors (it shares its stream start with the next one: the position search of
             k_select_mfma against the serial writers); one query sits on the duplicates, one on the empty list's centroid
  NaN        a query with a NaN element takes the canonical branch on route (b) by itself (the counter moves by one); (b) against (c)
  many lists 5000 and 17000 lists at dim 64 (k_select_mfma<1>: the score row in LDS, <0>: re-read from global memory), nprobe 40,
             48 queries, (b) against (c) only: route (a)'s all-pairs ranking is the slow one and adds nothing there
  portable   one base case under the numeric variant "portable" (the unfused first operation of block_lbmin), all three routes
The canonical sums' scalar tail Dmain..D needs a padded dimension that is no multiple of 8.  No index has one: FHT-Kac pads to a
multiple of 64 and the matrix rotator takes multiples of 16 only (tests/test_gpu_dim_edges.py), so that case does not exist here.
k_probes_given keeps its coverage from tests/test_gpu_mstg_search.py and the MSTG parity tests."""
import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import make_dataset

pytestmark = pytest.mark.gpu

N, NLIST, BITS, TOP_K, NQ = 2000, 16, 7, 10, 5
ROUTES = {"a": {"exact_rank": 1, "force_rank_fallback": 0}, "b": {"exact_rank": 0, "force_rank_fallback": 0},
          "c": {"exact_rank": 0, "force_rank_fallback": 1}}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what):
    bad = np.argwhere(_bits(a) != _bits(b))
    assert bad.size == 0, f"{what}: {len(bad)} element(s) differ, first at {bad[0].tolist()}: {_bits(a)[tuple(bad[0])]:#x} vs {_bits(b)[tuple(bad[0])]:#x}"


class _Runner:
    def __init__(self, built, variant=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.idx = rq.IvfRabitqIndex.from_built(built)
        self.idx.set_option("lazy_select", 0)
        if variant:
            self.idx.set_numeric_variant(variant)
        self.st = torch.cuda.Stream(self.dev)
        self.nblk = np.sort((built.list_sizes() + 31) // 32)[::-1]
        self.nlist = built.n_lists

    def run(self, route, q, nprobe):
        """one call under route's options: the stage resources, how far the fallback counter moved, what the selection wrote, the results"""
        torch, idx, s = self.torch, self.idx, self.st.cuda_stream
        for k, v in ROUTES[route].items():
            idx.set_option(k, v)
        nq, ws = len(q), max(int(self.nblk[:nprobe].sum()), 1)
        qd = torch.from_numpy(np.ascontiguousarray(q)).to(self.dev)
        ids = torch.zeros(nq, TOP_K, dtype=torch.int64, device=self.dev)
        sc = torch.zeros(nq, TOP_K, dtype=torch.float32, device=self.dev)
        cnt = torch.zeros(nq, dtype=torch.int32, device=self.dev)
        before = idx.rank_fallbacks()
        torch.cuda.synchronize(self.dev)
        idx.search_batch_device(qd.data_ptr(), nq, q.shape[1], TOP_K, nprobe, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), stream=s)
        torch.cuda.synchronize(self.dev)
        out = {"res": idx.stage_resources(nq, TOP_K, nprobe), "fallbacks": idx.rank_fallbacks() - before,
               "probe": idx.debug_copy_workspace(s, "probe", np.empty((nq, nprobe, 4), np.uint32)),
               "nstream": idx.debug_copy_workspace(s, "nstream", np.empty(nq, np.uint32)),
               "nvec": idx.debug_copy_workspace(s, "nvec", np.empty(nq, np.uint64)),
               "wl": idx.debug_copy_workspace(s, "wl", np.empty((nq, ws, 4), np.uint32)),
               "ids": ids.cpu().numpy(), "scores": sc.cpu().numpy(), "counts": cnt.cpu().numpy()}
        # the route: (a) ranks every pair in f32 on k_rank_scores' 32 x 32 tiles, (b) and (c) on the GEMM (every padded dim here is a
        # multiple of 64) and select with one kernel, which is not (a)'s
        rank = out["res"]["rank"]
        if route == "a":
            assert rank["operands"] == "f32" and rank["workgroups"] == ((self.nlist + 31) // 32) * ((nq + 31) // 32), rank
        else:
            assert rank["operands"] in ("bf16x3", "f16") and rank["workgroups"] > 0, rank
        assert out["res"]["select"]["workgroups"] == nq and out["res"]["select"]["threads"] == 256
        assert (out["nstream"] <= ws).all()
        return out

    def close(self):
        self.idx.release_stream(self.st.cuda_stream)
        self.idx.close()


def _agree(x, y, what):
    for name in ("probe", "nstream", "nvec", "ids", "scores", "counts"):
        _same(x[name], y[name], f"{what}: {name}")
    for i, ns in enumerate(x["nstream"]):
        _same(x["wl"][i, :ns], y["wl"][i, :ns], f"{what}: wl of query {i}")


def _three_routes(r, q, nprobe, what):
    """(a), (b), (c) on one batch; returns (b)'s output"""
    out = {k: r.run(k, q, nprobe) for k in ROUTES}
    assert out["a"]["fallbacks"] == 0 and out["b"]["fallbacks"] == 0 and out["c"]["fallbacks"] == len(q), {k: v["fallbacks"] for k, v in out.items()}
    sel = {k: (v["res"]["select"]["vgprs"], v["res"]["select"]["lds_bytes"]) for k, v in out.items()}
    assert sel["b"] == sel["c"] and sel["a"] != sel["b"], sel
    _agree(out["a"], out["b"], f"{what}: k_select vs k_select_mfma")
    _agree(out["b"], out["c"], f"{what}: k_select_mfma vs its canonical branch")
    return out["b"]


def _clusters(dim, metric, seed):
    data = make_dataset(N, dim, 4, seed, normalize=(metric == 1))
    cent, assign = rq.builder.kmeans(data, NLIST, 5, seed + 1)
    return data, np.ascontiguousarray(cent, np.float32), np.asarray(assign, np.uint32)


def _build(data, cent, assign, metric, seed):
    return rq.builder.train_with_clusters(data, cent, assign, BITS, metric, 1, seed, True)


@pytest.mark.parametrize("dim,metric", [(64, 0), (64, 1), (100, 0), (100, 1)], ids=["d64_L2", "d64_IP", "d100_pad128_L2", "d100_pad128_IP"])
def test_three_routes_agree(dim, metric):
    data, cent, assign = _clusters(dim, metric, 9500 + dim + metric)
    built = _build(data, cent, assign, metric, 9600 + dim)
    assert built.padded_dim % 64 == 0
    q = make_dataset(NQ, dim, 4, 9700 + dim, normalize=(metric == 1))
    q[4] = cent[2]
    r = _Runner(built)
    for nprobe in (4, NLIST):
        b = _three_routes(r, q, nprobe, f"dim {dim} metric {metric} nprobe {nprobe}")
        assert b["probe"][4, 0, 3] == 2 or metric == 1  # (L2: the query on centroid 2 probes list 2 first)
        if nprobe == NLIST:  # every list, once
            assert (np.sort(b["probe"][:, :, 3], axis=1) == np.arange(NLIST)).all()
            assert (b["nvec"] == N).all()
    # a query with a NaN element: the canonical branch by itself
    qn = q.copy()  # (five queries again: a call of up to four takes the latency front and has no GEMM)
    qn[0, 5] = np.nan
    b, c = r.run("b", qn, 4), r.run("c", qn, 4)
    assert b["fallbacks"] == 1 and c["fallbacks"] == NQ, (b["fallbacks"], c["fallbacks"])
    _agree(b, c, f"dim {dim} metric {metric}: NaN query, k_select_mfma vs its canonical branch")
    r.close()


@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_duplicate_centroids_and_an_empty_list(metric):
    dim = 64
    data, cent, assign = _clusters(dim, metric, 9800 + metric)
    q = make_dataset(NQ, dim, 4, 9820, normalize=(metric == 1))

    def order(v):  # the lists by the metric, best first (float64, unrotated: the margins at the top are wide)
        c, v = cent.astype(np.float64), v.astype(np.float64)
        return np.argsort(((c - v) ** 2).sum(axis=1) if metric == 0 else -(c @ v), kind="stable")

    # the two best lists of query 0 get the same centroid and share out the vectors of both
    t, u = (int(x) for x in order(q[0])[:2])
    cent[u] = cent[t]
    lo, hi = min(t, u), max(t, u)
    both = np.nonzero((assign == t) | (assign == u))[0]
    assign[both[0::2]], assign[both[1::2]] = lo, hi
    # the best other list of query 1 gives its vectors to the list of the nearest other centroid and stays empty
    e = int([x for x in order(q[1]) if x not in (t, u)][0])
    mine = np.nonzero(assign == e)[0]
    d2 = ((data[mine, None, :].astype(np.float64) - cent[None, :, :]) ** 2).sum(axis=2)
    d2[:, e] = np.inf
    assign[mine] = d2.argmin(axis=1).astype(np.uint32)
    built = _build(data, cent, assign, metric, 9810)
    sizes = built.list_sizes()
    assert sizes[e] == 0 and sizes[lo] > 0 and sizes[hi] > 0
    r = _Runner(built)
    for nprobe in (4, NLIST):
        b = _three_routes(r, q, nprobe, f"ties metric {metric} nprobe {nprobe}")
        cids = b["probe"][:, :, 3]
        for i in range(NQ):  # the duplicates are neighbours in the probe order, the smaller id first
            pl, ph = np.nonzero(cids[i] == lo)[0], np.nonzero(cids[i] == hi)[0]
            assert (len(pl), len(ph)) in ((0, 0), (1, 0), (1, 1)) and (len(ph) == 0 or ph[0] == pl[0] + 1), cids[i]
            if len(ph):
                _same(b["probe"][i, pl[0], :3], b["probe"][i, ph[0], :3], f"query {i}: constants of the duplicate centroids")
        assert list(cids[0, :2]) == [lo, hi] and e in cids[1, :3]  # the tie and the empty list are probed
    r.close()


@pytest.mark.parametrize("nlist", [5000, 17000], ids=["row_in_lds", "row_in_global"])
def test_many_lists_approximate_path_and_canonical_branch_agree(nlist):
    """built as test_gpu_parity.py::test_many_lists_select_row_modes builds its indexes"""
    import torch
    dim, n, nprobe = 64, 3 * nlist, 40
    data = make_dataset(n, dim, 64, 31)
    rng = np.random.default_rng(32)
    cent = data[rng.choice(n, nlist, replace=False)].copy()
    x, c = torch.from_numpy(data).cuda(), torch.from_numpy(cent).cuda()
    assign = torch.cdist(x, c).argmin(dim=1).cpu().numpy().astype(np.uint32)
    del x, c
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 33, True)
    q = make_dataset(48, dim, 64, 34)
    r = _Runner(built)
    b, c = r.run("b", q, nprobe), r.run("c", q, nprobe)
    assert b["fallbacks"] == 0 and c["fallbacks"] == len(q), (b["fallbacks"], c["fallbacks"])
    lds = b["res"]["select"]["lds_bytes"]
    assert lds == c["res"]["select"]["lds_bytes"] and (lds >= 4 * nlist) == (nlist == 5000), lds  # the score row is in LDS at 5000 lists only
    _agree(b, c, f"{nlist} lists: k_select_mfma vs its canonical branch")
    r.close()


def test_three_routes_agree_portable_variant():
    data, cent, assign = _clusters(64, 0, 9900)
    built = _build(data, cent, assign, 0, 9910)
    q = make_dataset(NQ, 64, 4, 9920)
    q[4] = cent[2]
    r = _Runner(built, "portable")
    _three_routes(r, q, 4, "portable, dim 64")
    r.close()
