"""What the range searches of the three index modules (index.py, mstg.py, bruteforce.py) share on the Python side."""
import numpy as np


def f32_bits(v):
    """The bit pattern of v as an f32, the form in which the handles' radius options take a float."""
    return int(np.array([v], np.float32).view(np.int32)[0])


def filter_words(allowed_ids):
    """The dense id bitset of a filter: (words [ceil(nbits / 32), at least 1] u32, nbits = largest id + 1)."""
    allowed = np.asarray(sorted(set(int(i) for i in allowed_ids)), dtype=np.uint64)
    nbits = int(allowed.max()) + 1 if allowed.size else 0
    words = np.zeros((nbits + 31) // 32 or 1, np.uint32)
    if allowed.size:
        np.bitwise_or.at(words, (allowed >> np.uint64(5)).astype(np.int64),
                         (np.uint32(1) << (allowed & np.uint64(31)).astype(np.uint32)))
    return words, nbits


def complete_rows(call, max_results):
    """call(cap) -> (ids, scores, totals, ...) with rows of capacity cap.  max_results=m: call(m) as it is.  None: complete rows — a
    first call with rows of 1024; where a total exceeds that, one more with rows of the largest total (the totals are exact, so
    one repeat suffices)."""
    cap = max_results or 1024
    got = call(cap)
    if max_results is None and got[2].size and int(got[2].max()) > cap:
        got = call(int(got[2].max()))
    return got


def csr(ids, scores, counts, sort):
    """Rows of capacity cap with their totals -> FAISS's (lims [nq + 1], ids, scores); a row holds min(total, cap)."""
    kept = np.minimum(counts.astype(np.int64), ids.shape[1])
    lims = np.zeros(len(kept) + 1, np.int64)
    np.cumsum(kept, out=lims[1:])
    take = np.arange(ids.shape[1])[None, :] < kept[:, None]
    out_ids, out_sc = ids[take], scores[take]  # (row-major: rows in query order, scan order inside a row)
    if sort:
        for q in range(len(kept)):
            o = np.argsort(out_sc[lims[q]:lims[q + 1]], kind="stable")  # (score, scan order)
            out_ids[lims[q]:lims[q + 1]] = out_ids[lims[q]:lims[q + 1]][o]
            out_sc[lims[q]:lims[q + 1]] = out_sc[lims[q]:lims[q + 1]][o]
    return lims, out_ids, out_sc
