"""The brute-force range search restated per query over bf_ref (the float32 restatement of the crate's distances): a vector
matches iff its distance is finite and below the radius; matches in id order; the row cut to `capacity` and padded."""
import numpy as np

import bf_ref

U64MAX = np.iinfo(np.uint64).max


def row(prep, q, r, capacity=None, allowed=None, d=None):
    """(ids u64 [capacity], scores f32 [capacity], total) for one query; capacity None: the complete row, unpadded"""
    d = bf_ref.distances(prep, q).astype(np.float32) if d is None else d
    keep = np.isfinite(d) & (d < np.float32(r))
    if allowed is not None:
        keep &= allowed
    ids = np.nonzero(keep)[0].astype(np.uint64)
    scores = (d[keep] if prep.metric == 0 else -d[keep]).astype(np.float32)
    if capacity is None:
        return ids, scores, len(ids)
    out_ids, out_sc = np.full(capacity, U64MAX, np.uint64), np.full(capacity, np.nan, np.float32)
    c = min(len(ids), capacity)
    out_ids[:c], out_sc[:c] = ids[:c], scores[:c]
    return out_ids, out_sc, len(ids)
