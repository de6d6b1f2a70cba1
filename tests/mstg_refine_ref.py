"""NumPy restatement of the refined MSTG search (include/rbq_mstg.h, rbq_mstg_search_refined_batch) over
the CPU oracle, and the cases its tests share.  No GPU.

An MSTG index is held by the oracle as the CPU builder's index over the expanded (vector, list) pairs: the oracle's ids are pair
indices and `pair_vec` maps them to the real ids.  Per selected list the oracle's own per-block code (`oracle.list_vectors`)
gives every vector's binary estimate `est` and refined distance `dist` (src/ivf.rs:2086-2099; `est` itself when ex_bits == 0);
steps 1 to 4 of the contract are then applied literally."""
import numpy as np

import oracle
import rabitq_rs_amd as rq
from rabitq_rs_amd import mstg

NONE64 = np.iinfo(np.uint64).max


class Case:
    """x [n][dim], c [k][dim], the closure's pairs, and the CPU builder's index over them (ids = pair indices)"""

    def __init__(self, x, c, bits, metric, eps, max_replicas, faster=True, pairs=None):
        self.x, self.c = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)
        self.bits, self.metric, self.eps, self.max_replicas, self.faster = bits, metric, eps, max_replicas, faster
        if pairs is None:
            lists, counts = rq.closure_assign_cpu(self.x, self.c, eps, max_replicas)
            pairs = mstg.expand_pairs(lists, counts)
        self.pair_vec, self.pair_list = pairs
        self.built = rq.builder.train_with_clusters(self.x[self.pair_vec], self.c, self.pair_list, bits, metric,
                                                    rq.RotatorType.NoRotation, 42, faster)

    def built_with_real_ids(self):
        """A second index over the same pairs whose stored ids are the real vector ids (what a device-built handle holds)."""
        b = rq.builder.train_with_clusters(self.x[self.pair_vec], self.c, self.pair_list, self.bits, self.metric,
                                           rq.RotatorType.NoRotation, 42, self.faster)
        pv = np.asarray(self.pair_vec)
        for cid in range(b.n_lists):
            lv = b.lists_ptr[cid]
            if lv.n:
                ids = np.ctypeslib.as_array(lv.ids, shape=(lv.n,))
                ids[:] = pv[ids.astype(np.int64)].astype(np.uint64)
        return b

    def device_index(self, **kw):
        return rq.build_postings_on_device(self.x, self.c, self.bits, self.metric, closure_epsilon=self.eps,
                                           max_replicas=self.max_replicas, faster_config=self.faster, **kw)


def candidates(built, pair_vec, q, lists_row, n_lists):
    """Every (list, position) entry of one query in (list order, vector order): (ids u64, est f32, dist f32), nothing dropped."""
    ids, est, dist = [], [], []
    q = np.ascontiguousarray(q, np.float32)
    for cid in lists_row[:int(n_lists)]:
        cid = int(cid)
        if int(built.lists_ptr[cid].n) == 0:
            continue
        g_add, _ = oracle.probe_geometry(built, q, cid)
        lv = oracle.list_vectors(built, q, cid, g_add, 0)
        ids.append(np.asarray(pair_vec)[built.list_ids(cid).astype(np.int64)].astype(np.uint64))
        est.append(lv["est"])
        dist.append(lv["dist"])
    if not ids:
        return np.zeros(0, np.uint64), np.zeros(0, np.float32), np.zeros(0, np.float32)
    return np.concatenate(ids), np.concatenate(est), np.concatenate(dist)


def binary_pool(est, metric, pool):
    """Step 1: indices (into the candidate arrays) of the pool in rank order, and their reported estimates.  Non-finite
    estimates are dropped, L2 estimates clamped; ascending by value, the earlier (list order, vector order) first among equals.
    `tie_at_cut`: an estimate equal to the last one taken was left out (which of the two a heap keeps is then a matter of its
    pushes and pops: the tests' data must not depend on it)."""
    keep = np.nonzero(np.isfinite(est))[0]
    e = est[keep]
    if metric == 0:
        e = np.where(e > 0, e, np.float32(0)).astype(np.float32)
    order = np.argsort(e, kind="stable")
    take = order[:pool]
    tie_at_cut = len(order) > pool and pool > 0 and e[order[pool]] == e[order[pool - 1]]
    return keep[take], e[take], bool(tie_at_cut)


def refine_query(ids, est, dist, metric, top_k, refine_pool):
    """Steps 1 to 4 for one query: (ids [top_k], scores [top_k], count, binary pool (ids, estimates), tie_at_cut)."""
    pool = max(int(refine_pool), int(top_k))
    sel, e, tie = binary_pool(est, metric, pool)
    d = dist[sel].astype(np.float32)
    pid = ids[sel]
    rank = np.arange(len(sel))
    fin = np.isfinite(d)                                    # a non-finite refined distance drops the candidate
    d, pid, rank = d[fin], pid[fin], rank[fin]
    if metric == 0:
        d = np.where(d > 0, d, np.float32(0)).astype(np.float32)
    # step 3: per id the smallest distance, then the smallest rank (lexsort: last key first; float keys compare by value)
    o = np.lexsort((rank, d, pid))
    first = np.ones(len(o), bool)
    first[1:] = pid[o][1:] != pid[o][:-1]
    o = o[first]
    d, pid, rank = d[o], pid[o], rank[o]
    # step 4
    o = np.lexsort((rank, d))[:top_k]
    out_ids = np.full(top_k, NONE64, np.uint64)
    out_sc = np.full(top_k, np.nan, np.float32)
    out_ids[:len(o)] = pid[o]
    out_sc[:len(o)] = d[o]
    return out_ids, out_sc, len(o), (ids[sel], e), tie


def refine_ref(built, pair_vec, queries, lists, counts, metric, top_k, refine_pool, cands=None):
    """The whole call: ids [nq][top_k], scores, counts, and per query the binary pool and whether a tie sat at its cut.
    `cands`: the per-query `candidates` of an earlier call over the same queries and lists (they do not depend on top_k or pool)."""
    q = np.ascontiguousarray(queries, np.float32)
    nq = len(q)
    ids = np.full((nq, top_k), NONE64, np.uint64)
    sc = np.full((nq, top_k), np.nan, np.float32)
    cnt = np.zeros(nq, np.uint32)
    pools, ties = [], []
    for i in range(nq):
        cid, est, dist = cands[i] if cands is not None else candidates(built, pair_vec, q[i], lists[i], counts[i])
        ids[i], sc[i], cnt[i], p, t = refine_query(cid, est, dist, metric, top_k, refine_pool)
        pools.append(p)
        ties.append(t)
    return ids, sc, cnt, pools, ties


def all_candidates(built, pair_vec, queries, lists, counts):
    q = np.ascontiguousarray(queries, np.float32)
    return [candidates(built, pair_vec, q[i], lists[i], counts[i]) for i in range(len(q))]


def explicit_case(x, c, assign, bits, metric):
    """every vector in exactly one list (`assign`): IvfRabitqIndex.from_built(case.built_with_real_ids()) is its handle"""
    order = np.lexsort((np.arange(len(assign)), assign))
    return Case(x, c, bits, metric, 0.0, 1, pairs=(order.astype(np.int64), np.asarray(assign, np.uint32)[order]))


def list_length_case(bits, metric, dim=64, seed=3):
    """four lists of 0, 1, 32 and 33 vectors: a last block with 1 valid lane, a full one, a full one followed by 1 lane"""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 32, 33]
    c = (rng.standard_normal((4, dim)) * 2).astype(np.float32)
    assign = np.repeat(np.arange(4), sizes).astype(np.uint32)
    x = (c[assign] + 0.3 * rng.standard_normal((len(assign), dim))).astype(np.float32)
    q = (x[rng.integers(0, len(x), 8)] + 0.05 * rng.standard_normal((8, dim))).astype(np.float32)
    return explicit_case(x, c, assign, bits, metric), q


def exact_tie_case(bits, metric, dim=32, m=60, seed=4):
    """every vector twice under different ids: ids i and m + i hold the same vector, in the same list for even i (equal estimates
    and equal refined distances: rank decides) and in two different lists for odd i"""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((4, dim)) * 2).astype(np.float32)
    a0 = rng.integers(0, 4, m)
    base = (c[a0] + 0.3 * rng.standard_normal((m, dim))).astype(np.float32)
    x = np.concatenate([base, base])
    assign = np.concatenate([a0, np.where(np.arange(m) % 2 == 0, a0, (a0 + 1) % 4)]).astype(np.uint32)
    q = (base[rng.integers(0, m, 12)] + 0.05 * rng.standard_normal((12, dim))).astype(np.float32)
    return explicit_case(x, c, assign, bits, metric), q


def main_case(bits, metric):
    """The main case of the GPU test: n 1500, dim 64, 24 lists, closure epsilon 2.0, max_replicas 8; 48 queries near data points."""
    import closure_cases as cc
    n, dim, k = 1500, 64, 24
    x, c = cc.clustered(n, dim, k, 300 + bits)
    case = Case(x, c, bits, metric, 2.0, 8)
    rng = np.random.default_rng(5)
    q = (x[rng.integers(0, n, 48)] + 0.01 * rng.standard_normal((48, dim))).astype(np.float32)
    return case, q


def recall_case():
    """The fixed 7-bit L2 case of the recall figures: 4000 clustered vectors in 64 dimensions, 64 lists, the crate's closure
    epsilon; 64 queries a little off data points."""
    import closure_cases as cc
    n, dim, k = 4000, 64, 64
    x, c = cc.clustered(n, dim, k, 77, intrinsic=8, noise=0.05)
    case = Case(x, c, 7, 0, 0.15, 8)
    rng = np.random.default_rng(78)
    q = (x[rng.integers(0, n, 64)] + 0.05 * rng.standard_normal((64, dim))).astype(np.float32)
    return case, q


def recall_at(ids, counts, truth):
    """mean over the queries of |distinct returned ids that are true neighbours| / k"""
    k = truth.shape[1]
    hit = 0
    for i in range(len(truth)):
        hit += len(set(ids[i, :int(counts[i])].tolist()) & set(truth[i].tolist()))
    return hit / (len(truth) * k)
