"""Every way a replica's device arrays come into being, against each other (csrc/host/rbq_index_layout.hpp):
one tiny data set, dim 64, FHT-Kac, 8 lists of [0, 1, 31, 32, 33, 64, 65, 5] vectors, at ex_bits 0, 2 and 6, is turned into an
IVF handle over eight routes and into an MSTG handle over three, and every array rbq_debug_copy_index serves is compared with the
first route's: the list tables, the centroid arrays and the block / list summaries as a whole, the per-slot arrays on the real
slots, and a search's ids and score bits.  Every comparison is exact.

Pad slots (the slots of a list's last block past its size).  No result depends on them, so a route is free to leave other
bytes there.  PADS_AGREE / MSTG_PADS_AGREE record, route by route, the per-slot arrays whose pad slots equal the first route's.
That is a fact, not a choice: it was read off the tree as it stood before the construction paths shared one layout and one
allocation (_pad_agreement computes it), at ex_bits 0, 2 and 6 alike:
  IVF   every route agrees with from_built on the pad slots of every per-slot array it holds — blocks, ids, ex, fadd_ex, fres_ex,
        delta, vl (from_built_without_recon holds no delta / vl)
  MSTG  load and append-then-remove agree with the one-shot build on the pad slots of all of those and of rnorm
A route may only ever be added to these tables."""
import ctypes as C
import functools
import io
import re

import numpy as np
import pytest
import torch

import closure_cases as cc
import rabitq_rs_amd as rq
from conftest import make_dataset
from rabitq_rs_amd import mstg
from rabitq_rs_amd.index import _detail, lib

pytestmark = pytest.mark.gpu

DIM, SIZES, EXTRA = 64, [0, 1, 31, 32, 33, 64, 65, 5], 40
N, NL = sum(SIZES), len(SIZES)
WHOLE = ("list_gb0", "list_n", "centroids", "cnorm2", "bsum", "lsum", "bsumx", "cent_hl", "cent_hi", "cent_lo", "cent_f16",
         "cent_f16_resid")
SLOT = ("blocks", "ids", "ex", "fadd_ex", "fres_ex", "delta", "vl", "rnorm")
IVF_ROUTES = ("from_built", "from_built_without_recon", "load_from_bytes", "load_from_reader", "build_on_device", "stream_builder",
              "add", "remove_ids")
MSTG_ROUTES = ("build", "load", "append_remove")
ALL_SLOT = frozenset(SLOT)
# route -> the per-slot arrays whose pad slots equal the first route's (module docstring)
PADS_AGREE = {r: ALL_SLOT - {"delta", "vl"} if r == "from_built_without_recon" else ALL_SLOT for r in IVF_ROUTES}
MSTG_PADS_AGREE = {r: ALL_SLOT for r in MSTG_ROUTES}
EPS, M = 2.0, 8


def _arrays(idx):
    """name -> bytes of every array the handle serves (the library says how long each is; an array it does not hold is empty)"""
    out = {}
    for name in WHOLE + SLOT:
        rc = lib().rbq_debug_copy_index(idx._h, name.encode(), C.byref(C.c_uint8()), 0)
        n = 0 if rc == 0 else int(re.search(r"have (\d+) bytes", _detail()).group(1))
        buf = np.empty(n, np.uint8)
        if n:
            idx.debug_copy_index(name, buf)
        out[name] = buf
    return out


def _block_slot_bytes(Dc):
    """[32][bytes per slot] offsets inside a block record of the bytes that belong to slot v: its sign code (16 bytes per group
    of 128 dimensions, 8 in a last group of 64) and its three factors"""
    G16, tail = Dc // 128, Dc % 128 == 64
    rows = []
    for v in range(32):
        o = [g * 512 + v * 16 + j for g in range(G16) for j in range(16)]
        o += [G16 * 512 + v * 8 + j for j in range(8)] if tail else []
        o += [4 * Dc + k * 128 + v * 4 + j for k in range(3) for j in range(4)]
        rows.append(o)
    return np.asarray(rows, np.int64)


def _per_slot(name, buf, nslots, Dc):
    """[nslots][bytes of one slot] view (a gather for `blocks`) of a per-slot array"""
    if name == "blocks":
        stride = 4 * Dc + 384
        assert buf.size == nslots // 32 * stride
        sb = _block_slot_bytes(Dc)
        assert np.array_equal(np.sort(sb.ravel()), np.arange(stride)), "every byte of a block record belongs to one slot"
        return buf.reshape(nslots // 32, stride)[:, sb].reshape(nslots, sb.shape[1])
    assert buf.size % nslots == 0
    return buf.reshape(nslots, buf.size // nslots)


def _slot_masks(ref):
    gb0, ln = ref["list_gb0"].view(np.uint32).astype(np.int64), ref["list_n"].view(np.uint32).astype(np.int64)
    nslots = int(((ln + 31) // 32).sum()) * 32
    real = np.zeros(nslots, bool)
    for g, n in zip(gb0, ln):
        real[g * 32:g * 32 + n] = True
    return nslots, real


def _compare(ref, got, pads_agree, what):
    """the contract of the module docstring between two handles' arrays; returns the per-slot arrays whose pad slots agree"""
    nslots, real = _slot_masks(ref)
    assert nslots and real.any() and (~real).any()
    Dc = (DIM + 63) // 64 * 64
    for name in WHOLE:
        assert ref[name].size and np.array_equal(ref[name], got[name]), (what, name)
    agree = set()
    for name in SLOT:
        if not got[name].size:  # not held by this route (delta / vl without factors) or by any (ex at ex_bits 0, rnorm on IVF)
            assert name not in pads_agree or not ref[name].size, (what, name, "held by the first route only")
            continue
        assert ref[name].size == got[name].size, (what, name, ref[name].size, got[name].size)
        a, b = _per_slot(name, ref[name], nslots, Dc), _per_slot(name, got[name], nslots, Dc)
        assert np.array_equal(a[real], b[real]), (what, name, "real slots")
        if np.array_equal(a[~real], b[~real]):
            agree.add(name)
        assert name in agree or name not in pads_agree, (what, name, "pad slots")
    return agree


class Ivf:
    """the data set and its eight handles at one ex_bits; the first route is the reference of the others"""

    def __init__(self, bits):
        rng = np.random.default_rng(3600 + bits)
        self.data = make_dataset(N + EXTRA, DIM, 4, 3601 + bits)
        a = rng.permutation(np.repeat(np.arange(NL), SIZES))
        self.assign = np.concatenate([a, rng.integers(0, NL, EXTRA)]).astype(np.uint32)
        self.cent = np.stack([self.data[:N][a == c].mean(0) if (a == c).any() else self.data[c] for c in range(NL)]).astype(np.float32)
        self.built = rq.builder.train_with_clusters(self.data[:N], self.cent, self.assign[:N], bits, 0, 1, 3602 + bits, True)
        self.t = self.built.t_const
        self.xd = torch.from_numpy(self.data).cuda()
        self.ad = torch.from_numpy(self.assign.astype(np.int32)).cuda()
        self.q = make_dataset(4, DIM, 4, 3603 + bits)

    def _device(self, n):
        return rq.IvfRabitqIndex.build_on_device(self.built.hdr_ptr, self.cent, self.xd.data_ptr(), self.ad.data_ptr(), n, self.t)

    def route(self, name):
        if name == "from_built":
            return rq.IvfRabitqIndex.from_built(self.built)
        if name == "from_built_without_recon":
            return rq.IvfRabitqIndex.from_built_without_recon(self.built)
        if name in ("load_from_bytes", "load_from_reader"):
            src = rq.IvfRabitqIndex.from_built(self.built)
            raw = src.save_to_bytes()
            src.close()
            return rq.IvfRabitqIndex.load_from_bytes(raw) if name == "load_from_bytes" else rq.IvfRabitqIndex.load_from_reader(io.BytesIO(raw))
        if name == "build_on_device":
            return self._device(N)
        h = N // 2
        if name == "stream_builder":
            b = rq.StreamBuilder(self.built.hdr_ptr, self.cent, SIZES, self.t)
            b.push(self.data[:h], self.assign[:h], 0)
            b.push(self.data[h:N], self.assign[h:N], h)
            return b.finish()
        if name == "add":
            idx = self._device(h)
            got = idx.add(self.xd[h:N], self.ad[h:N], first_id=h)
            assert np.array_equal(got, self.assign[h:N])
            return idx
        assert name == "remove_ids"
        idx = self._device(N + EXTRA)
        assert idx.remove_ids(np.arange(N, N + EXTRA, dtype=np.uint64)) == EXTRA
        return idx

    def answers(self, idx):
        ids, sc, cnt, _ = idx.batch_search_raw(self.q, rq.SearchParams(5, NL))
        return ids.tobytes(), sc.tobytes(), cnt.tobytes()


class Mstg:
    """the posting-list handle of the same shape over its three routes"""

    def __init__(self, bits):
        self.bits = bits
        self.x, self.c = _mstg_data()
        self.cfg = rq.MstgIndex(DIM, "euclidean", closure_epsilon=EPS, max_replicas=M, rabitq_bits=bits, faster_config=True).config()
        rng = np.random.default_rng(3700 + bits)
        self.q = (self.x[rng.integers(0, N, 4)] + 0.01 * rng.standard_normal((4, DIM))).astype(np.float32)

    def _build(self, n):
        return rq.build_postings_on_device(self.x[:n], self.c, self.bits, 0, closure_epsilon=EPS, max_replicas=M, faster_config=True)

    def route(self, name):
        if name == "build":
            return self._build(N)
        if name == "load":
            src = self._build(N)
            raw = mstg.save_mstg_bytes(src, self.cfg)
            src.close()
            return mstg.load_mstg(raw)[0]
        assert name == "append_remove"
        base = self._build(N)
        grown = mstg.append_postings(base, self.x[N:], closure_epsilon=EPS, max_replicas=M)
        assert len(grown) > len(base) and grown.id_bound() == N + EXTRA
        got, removed = mstg.remove_postings(grown, np.arange(N, N + EXTRA, dtype=np.uint64))
        assert removed == len(grown) - len(base)
        base.close(); grown.close()
        return got

    def answers(self, idx):
        out = []
        for pool in (None, 64):
            ids, sc, cnt = mstg.mstg_search(idx, self.q, 5, NL, 0.6, refine_pool=pool)
            keep = np.arange(5)[None, :] < cnt[:, None]
            out += [np.where(keep, ids, 0).tobytes(), np.where(keep, sc.view(np.uint32), 0).tobytes(), cnt.tobytes()]
        return tuple(out)


@functools.lru_cache(maxsize=None)
def _mstg_data():
    return cc.clustered(N + EXTRA, DIM, NL, 3710)  # shared by the three cases: computed once, never written


def _pad_agreement(case, routes):
    """route -> sorted per-slot arrays whose pad slots equal the first route's (what PADS_AGREE records)"""
    first = case.route(routes[0])
    ref = _arrays(first)
    out = {}
    for r in routes[1:]:
        idx = case.route(r)
        out[r] = sorted(_compare(ref, _arrays(idx), frozenset(), r))
        idx.close()
    first.close()
    return out


def _check_routes(case, routes, pads_agree):
    first = case.route(routes[0])
    ref, want = _arrays(first), case.answers(first)
    assert any(want), "the search found nothing"
    for r in routes[1:]:
        idx = case.route(r)
        assert len(idx) == len(first) and idx.cluster_count() == NL
        _compare(ref, _arrays(idx), pads_agree[r], r)
        assert case.answers(idx) == want, (r, "search ids / score bits / counts")
        idx.close()
    return ref, first


@pytest.mark.parametrize("bits", [1, 3, 7], ids=["ex0", "ex2", "ex6"])
def test_ivf_routes_build_the_same_arrays(bits):
    case = Ivf(bits)
    ref, first = _check_routes(case, IVF_ROUTES, PADS_AGREE)
    assert ref["list_n"].view(np.uint32).tolist() == SIZES and len(first) == N
    assert ref["list_gb0"].view(np.uint32).tolist() == [0, 0, 1, 2, 3, 5, 7, 10]
    assert ref["delta"].size and not ref["rnorm"].size and bool(ref["ex"].size) == (bits > 1)
    first.close()


@pytest.mark.parametrize("bits", [1, 3, 7], ids=["ex0", "ex2", "ex6"])
def test_mstg_routes_build_the_same_arrays(bits):
    case = Mstg(bits)
    ref, first = _check_routes(case, MSTG_ROUTES, MSTG_PADS_AGREE)
    ln = ref["list_n"].view(np.uint32)
    assert int(ln.sum()) == len(first) > N and (ln % 32 != 0).any(), "no replicated vector, or no partly filled block"
    assert ref["rnorm"].size == ref["delta"].size > 0
    first.close()
