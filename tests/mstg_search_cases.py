"""Cases and comparisons of tests/test_gpu_mstg_search.py: MSTG indexes built by the CPU builder with NoRotation (so that the
oracle holds the same lists), and the two assertions every case makes."""
import numpy as np

import oracle
import rabitq_rs_amd as rq
from conftest import make_dataset
from rabitq_rs_amd import mstg

NONE64 = np.iinfo(np.uint64).max


def kmeans_case(metric, bits, dim, n, nlist, nq, seed, offset=0.0):
    data = make_dataset(n, dim, 12, seed, normalize=(metric == 1))
    q = make_dataset(nq, dim, 12, seed + 1, normalize=(metric == 1))
    if offset:
        data, q = (data + offset).astype(np.float32), (q + offset).astype(np.float32)
    cent, assign = rq.builder.kmeans(data, nlist, 3, seed)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rq.RotatorType.NoRotation, seed, True)
    return built, np.ascontiguousarray(cent, np.float32), q


def pair_case(metric, bits, dim, nlist, nq, seed, offset=0.0, per_list=2):
    """nlist short lists: list c holds vectors per_list * c .. per_list * c + per_list - 1, its centroid is their mean"""
    rng = np.random.default_rng(seed)
    n = nlist * per_list
    base = rng.standard_normal((nlist, dim)).astype(np.float32) * 3
    data = (np.repeat(base, per_list, axis=0) + 0.3 * rng.standard_normal((n, dim)) + offset).astype(np.float32)
    cent = data.reshape(nlist, per_list, dim).mean(axis=1, dtype=np.float32)
    assign = (np.arange(n) // per_list).astype(np.uint32)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rq.RotatorType.NoRotation, seed, True)
    q = (data[rng.integers(0, n, nq)] + 0.2 * rng.standard_normal((nq, dim))).astype(np.float32)
    return built, cent, q


def given_centroids_case(bits, data, cent, seed, metric=0):
    """every vector goes to a list drawn at random: only the centroids matter to the selection"""
    rng = np.random.default_rng(seed)
    assign = rng.integers(0, len(cent), len(data)).astype(np.uint32)
    return rq.builder.train_with_clusters(data, cent, assign, bits, metric, rq.RotatorType.NoRotation, seed, True)


def check(idx, built, cent, q, top_k, ef_search, eps, metric):
    """The two assertions of every case; returns the search's outputs."""
    before = mstg.search_fallbacks()
    ids, sc, cnt, li, lc = rq.mstg_search(idx, q, top_k, ef_search, eps, return_lists=True)
    print(f"mstg_search: nq={len(q)} k={len(cent)} ef={ef_search} eps={eps} top_k={top_k} fallbacks={mstg.search_fallbacks() - before} "
          f"mean lists={lc.mean():.1f}")
    # 1. the selected lists and counts are select_lists_cpu's
    rl, rc = rq.select_lists_cpu(q, cent, ef_search, eps)
    assert np.array_equal(lc, rc), np.nonzero(lc != rc)[0][:10]
    bad = np.nonzero((li != rl).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], li[bad[0]], rl[bad[0]])
    if rl.shape[1] == 0:  # ef_search = 0: nothing to scan
        assert not cnt.any() and (ids == NONE64).all() and np.isnan(sc).all()
        return ids, sc, cnt, li, lc
    # 2a. ids, counts and score bits are rbq_posting_scan_batch's over those lists
    pids, psc, pcnt = idx.posting_scan(q, top_k, rl, rc)
    assert np.array_equal(cnt, pcnt) and np.array_equal(ids, pids)
    assert np.array_equal(sc.view(np.uint32), psc.view(np.uint32))
    # 2b. ... and the oracle's.  The reference partitions with select_nth_unstable_by on the distance alone, so among equal
    # distances which id is returned (and where) is not defined there: ids are compared where the distance is unique in the row
    # and differs from the last one returned; -0.0 and 0.0 are one L2 distance
    if built is not None:
        r, oids, osc, ocnt = oracle.posting_scan_batch(built, q, top_k, rl, rc)
        assert r == 0 and np.array_equal(cnt, ocnt)
        mask = np.uint32(0x7fffffff if metric == 0 else 0xffffffff)
        for i in range(len(q)):
            c = int(cnt[i])
            assert np.array_equal(sc[i, :c].view(np.uint32) & mask, osc[i, :c].view(np.uint32) & mask), i
            assert (ids[i, c:] == NONE64).all() and np.isnan(sc[i, c:]).all()
            if c:
                s = sc[i, :c]
                uniq = np.ones(c, bool)
                uniq[1:] &= s[1:] != s[:-1]
                uniq[:-1] &= s[:-1] != s[1:]
                uniq &= s != s[-1]
                assert np.array_equal(ids[i, :c][uniq], oids[i, :c][uniq]), i
    return ids, sc, cnt, li, lc
