"""Independent NumPy restatement of the list selection of the MSTG search (include/rbq_mstg.h, "the selection", steps 1-3).  It
shares no code with the host library: S comes from the oracle's ref_l2_distance_sqr, the square root, the threshold and the
stable order are computed in np.float32."""
import ctypes as C

import numpy as np

import oracle

NONE = 0xFFFFFFFF


def select_lists_ref(queries, centroids, ef_search, pruning_epsilon):
    q = np.ascontiguousarray(queries, np.float32)
    c = np.ascontiguousarray(centroids, np.float32)
    nq, dim = q.shape
    k = c.shape[0]
    ef = min(max(int(ef_search), 0), k)
    lists = np.full((nq, ef), NONE, np.uint32)
    counts = np.zeros(nq, np.uint32)
    f32p = C.POINTER(C.c_float)
    fn = oracle.lib().ref_l2_distance_sqr
    for i in range(nq):
        qp = q[i].ctypes.data_as(f32p)
        S = np.array([fn(qp, c[j].ctypes.data_as(f32p), dim) for j in range(k)], np.float32)
        if ef == 0 or np.isnan(S).any():
            continue
        # (bits of S, centroid index) ascending: S >= 0, so the bit patterns order like the values; stable = ties by index
        order = np.argsort(S.view(np.uint32), kind="stable")[:ef]
        if np.isinf(S[order[0]]):
            continue
        d = np.sqrt(S[order], dtype=np.float32)
        one_eps = np.float32(1.0) + np.float32(pruning_epsilon)
        with np.errstate(all="ignore"):
            thr = np.float32(d[0] * one_eps)
            keep = d <= thr
        n = int(keep.sum())
        assert keep[:n].all()  # a prefix: d is monotone in S
        lists[i, :n] = order[:n]
        counts[i] = n
    return lists, counts
