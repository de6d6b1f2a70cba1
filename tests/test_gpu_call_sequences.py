"""A search call's result must not depend on the calls the handle served before.  Every call writes nothing
in a workspace of its own: it runs on the Workspace of its stream (csrc/device/api.hpp), whose buffers only grow and are never
cleared, at strides that change from call to call.  The kinds of tests/call_sequence_cases.py run once each on a fresh handle and a
fresh stream — the ISOLATED result, checked against the CPU reference by the rule of the feature's own test — and then after every
other kind, in unsynchronised chains, on two streams, through the host entry and around refused calls; each result must equal the
isolated one bit for bit: ids, scores as uint32, counts, diagnostics and padding.  Run with `pytest -m gpu` on an MI355X."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import call_sequence_cases as cs
import rabitq_rs_amd as rq
from call_sequence_cases import BY_NAME, KINDS, ROUTES, Result, case, kinds_of, reference, same_bits
from rabitq_rs_amd import index as rq_index

pytestmark = pytest.mark.gpu

U64_FILL, U32_FILL = (int.from_bytes(bytes([cs.FILL]) * n, "little") for n in (8, 4))  # cs.FILL in every byte of every output buffer before a call


def _dev():
    import torch
    return torch.device("cuda", 0)


def open_handle(index, **kw):
    """a handle of an index; A and B with their raw vectors attached and the rerank OFF (the rerank kinds switch it on for their call)"""
    c = case(index)
    idx = rq.IvfRabitqIndex.from_built(c.built, **kw)
    if index in ("A", "B"):
        idx.set_rerank_vectors(c.data)
        idx.set_option("rerank", 0)
    return idx


def _set(idx, name, value):
    if name == "numeric_variant":
        idx.set_numeric_variant(value)
    else:
        idx.set_option(name, value)


@contextlib.contextmanager
def options(idx, kind):
    """the options of a kind, set for one call and put back after it, error or not; the caller keeps the stream idle around it"""
    done = []
    try:
        for name, value, back in kind.opts:
            _set(idx, name, value)
            done.append((name, back))
        if kind.mode == "range_exact":
            idx.set_range_exact(cs.radii(kind.name)[1])
        if kind.mode in ("range", "range_exact"):
            idx.set_range_search(cs.radii(kind.name)[0])
        yield
    finally:
        if kind.mode in ("range", "range_exact"):
            idx.set_range_search(None)
        if kind.mode == "range_exact":
            idx.set_range_exact(None)
        for name, back in reversed(done):
            _set(idx, name, back)


_INPUTS = {}


def dev_inputs(kind):
    """(queries, filter words | None, filter bits) of a kind in device memory, uploaded once per process"""
    import torch
    if kind.name not in _INPUTS:
        handed = cs.queries(kind)[0]
        qd = torch.from_numpy(np.ascontiguousarray(handed).view(np.uint8).reshape(-1).copy()).to(_dev())
        keep, fw, nbits = cs.filter_of(kind)
        fd = torch.from_numpy(fw.view(np.int32).copy()).to(_dev()) if fw is not None else None
        torch.cuda.synchronize(_dev())
        _INPUTS[kind.name] = (qd, fd, nbits)
    return _INPUTS[kind.name]


class Pending:
    """the output tensors of one device-entry call, filled with the pattern on the call's stream"""

    def __init__(self, kind, stream):
        import torch
        nq, k = kind.rows[1], reference(kind.name).top_k
        with torch.cuda.stream(stream):
            self.ids = torch.full((nq, k), U64_FILL, dtype=torch.int64, device=_dev())
            self.sc = torch.full((nq, k), U32_FILL, dtype=torch.int32, device=_dev())
            self.cnt = torch.full((nq,), U32_FILL, dtype=torch.int32, device=_dev())
            self.dg = torch.full((nq, 3), U64_FILL, dtype=torch.int64, device=_dev()) if kind.diag else None
        self.kind, self.k = kind, k

    def result(self):
        return Result(self.ids.cpu().numpy().view(np.uint64), self.sc.cpu().numpy().view(np.float32), self.cnt.cpu().numpy().view(np.uint32),
                      self.dg.cpu().numpy().view(np.uint64) if self.dg is not None else None)


def enqueue(idx, kind, stream, out=None):
    """rbq_search_batch_device of a kind on `stream`, no host synchronisation; the options are the caller's business"""
    out = out or Pending(kind, stream)
    qd, fd, nbits = dev_inputs(kind)
    dim = case(kind.index).q.shape[1]
    idx.search_batch_device(qd.data_ptr(), kind.rows[1], dim, out.k, kind.nprobe, out.ids.data_ptr(), out.sc.data_ptr(), out.cnt.data_ptr(),
                            stream=C.c_void_p(stream.cuda_stream), d_filter=fd.data_ptr() if fd is not None else None, filter_nbits=nbits,
                            d_diag=out.dg.data_ptr() if out.dg is not None else None)
    return out


def _host_buffers(nq, k, diag):
    return (np.full((nq, k), U64_FILL, np.uint64), np.full((nq, k), U32_FILL, np.uint32).view(np.float32), np.full(nq, U32_FILL, np.uint32),
            np.full((nq, 3), U64_FILL, np.uint64) if diag else None)


def run_host(idx, kind):
    """rbq_search_batch (or rbq_posting_scan_batch) of a kind from pageable buffers filled with the pattern"""
    L = rq_index.lib()
    handed = cs.queries(kind)[0]
    nq, k, dim = kind.rows[1], reference(kind.name).top_k, case(kind.index).q.shape[1]
    ids, sc, cnt, dg = _host_buffers(nq, k, kind.diag)
    if kind.mode == "posting":
        lists, counts = cs.posting_lists(kind)
        rc = L.rbq_posting_scan_batch(idx._h, handed.ctypes.data, nq, dim, k, lists.ctypes.data, counts.ctypes.data, lists.shape[1],
                                      ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    else:
        keep, fw, nbits = cs.filter_of(kind)
        rc = L.rbq_search_batch(idx._h, handed.ctypes.data, nq, dim, k, kind.nprobe, fw.ctypes.data if fw is not None else None, nbits,
                                ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, dg.ctypes.data if dg is not None else None)
    rq_index._check(rc)
    return Result(ids, sc, cnt, dg)


def run(idx, kind, stream, entry=None):
    """one call of a kind, its options set and put back around it with the stream idle; entry: the kind's own, or forced"""
    with options(idx, kind):
        if (entry or kind.entry) == "host" or kind.mode == "posting":
            return run_host(idx, kind)
        out = enqueue(idx, kind, stream)
        stream.synchronize()
        return out.result()


# ---- 1. isolated: a handle and a stream of its own, the route the stage probe reports, the CPU reference --------------------------
def assert_route(idx, kind):
    """rbq_debug_stage_resources (nothing runs) against ROUTES, with the kind's options set"""
    exp = ROUTES.get(kind.name)
    if exp is None:
        return
    nq, k = kind.rows[1], reference(kind.name).top_k
    inner_k = dict((o[0], o[1]) for o in kind.opts).get("rerank_pool", k)
    res = idx.stage_resources(nq, inner_k, kind.nprobe)
    what = f"{kind.name}: {res}"
    if "prep" in exp:
        assert res["prep"]["workgroups"] == exp["prep"], what
    if "rank" in exp:
        if exp["rank"] is None:  # a latency front shows no ranking stage
            assert res["rank"]["workgroups"] == 0, what
        else:
            assert res["rank"]["workgroups"] > 0 and res["rank"]["operands"] == exp["rank"], what
    assert res["scan"]["threads"] == exp["scan"], what
    if "parts" in exp:  # the GEMM's grid carries its parts in z: `parts` times the workgroups of the same call unsplit
        own = dict((o[0], o[1]) for o in kind.opts).get("rank_ksplit", 1)
        idx.set_option("rank_ksplit", 0)
        try:
            base = idx.stage_resources(nq, inner_k, kind.nprobe)
        finally:
            idx.set_option("rank_ksplit", own)
        assert res["rank"]["workgroups"] == exp["parts"] * base["rank"]["workgroups"], f"{what} unsplit: {base['rank']}"


_ISOLATED = {}


def isolated(name):
    """the isolated result of a kind, computed once per process and left unchanged"""
    import torch
    if name not in _ISOLATED:
        kind = BY_NAME[name]
        idx = open_handle(kind.index)
        st = torch.cuda.Stream(_dev())
        try:
            with options(idx, kind):
                assert_route(idx, kind)
            got = run(idx, kind, st)
            cs.check(kind, got)
            idx.release_stream(st.cuda_stream)
        finally:
            idx.close()
        for a in got:
            if a is not None:
                a.setflags(write=False)
        _ISOLATED[name] = got
    return _ISOLATED[name]


@pytest.mark.parametrize("name", [k.name for k in KINDS])
def test_isolated(name):
    isolated(name)


def test_rank_f16_qualifies():
    """the f16 kind is in the catalogue because index A's f16 image qualifies: with rank_f16 1 and no parts the probe names the f16 product"""
    idx = open_handle("A")
    try:
        idx.set_option("rank_f16", 1)
        idx.set_option("rank_ksplit", 0)
        assert idx.stage_resources(64, 10, 6)["rank"]["operands"] == "f16"
    finally:
        idx.close()


# ---- shared handles: one per index for the whole module (the longer a handle's history, the better) ------------------------------
_SHARED = {}


def shared(index):
    import torch
    if index not in _SHARED:
        _SHARED[index] = (open_handle(index), torch.cuda.Stream(_dev()))
    return _SHARED[index]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for idx, _ in _SHARED.values():
        idx.close()
    _SHARED.clear()
    _INPUTS.clear()


# ---- 2. every ordered pair (and 7: the posting-list handle) --------------------------------------------------------------------------
@pytest.mark.parametrize("first", [k.name for k in KINDS])
def test_after(first):
    """one handle, one stream: for every kind Y of the index, `first`, synchronise, Y — and Y answers as it does alone"""
    x = BY_NAME[first]
    idx, st = shared(x.index)
    for y in kinds_of(x.index):
        run(idx, x, st)
        same_bits(run(idx, y, st), isolated(y.name), f"{y.name} after {x.name}")


# ---- 3. unsynchronised chains on one stream ------------------------------------------------------------------------------------------
def _records(seq, key):
    """how often the running maximum of a call parameter grows after the first call of a chain"""
    best, n = key(seq[0]), 0
    for k in seq[1:]:
        if key(k) > best:
            best, n = key(k), n + 1
    return n


def chains(index):
    """three seeded permutations of the plain kinds; the first is ordered so that nq, nprobe and top_k each set a new maximum at
    least twice in mid-chain: Buf::ensure frees and reallocates while earlier calls are still queued"""
    plain = [k for k in kinds_of(index) if cs.plain(k)]
    grow = sorted(plain, key=lambda k: (k.rows[1] * k.top_k * k.nprobe, k.name))
    out = [grow]
    for seed in (3441, 3442):
        out.append([plain[i] for i in np.random.default_rng(seed).permutation(len(plain))])
    return out


def run_chain(idx, stream, seq):
    """enqueue `seq` back to back (own output tensors, allocated before the first call), synchronise once; the results"""
    outs = [Pending(k, stream) for k in seq]
    for k in seq:
        dev_inputs(k)
    for k, o in zip(seq, outs):
        enqueue(idx, k, stream, o)
    stream.synchronize()
    return [o.result() for o in outs]


@pytest.mark.parametrize("index", ["A", "B"])
def test_unsynchronised_chains(index):
    import torch
    seqs = chains(index)
    assert len(seqs[0]) >= 6
    for key in (lambda k: k.rows[1], lambda k: k.nprobe, lambda k: k.top_k):
        assert _records(seqs[0], key) >= 2, [k.name for k in seqs[0]]
    want = {k.name: isolated(k.name) for k in seqs[0]}
    idx = open_handle(index)
    st = torch.cuda.Stream(_dev())
    try:
        for n, seq in enumerate(seqs):
            for k, got in zip(seq, run_chain(idx, st, seq)):
                same_bits(got, want[k.name], f"chain {n}: {k.name} in {[s.name for s in seq]}")
    finally:
        idx.close()


@pytest.mark.parametrize("index", ["A", "B"])
def test_unsynchronised_range_chains(index):
    """the range option set once, then capacities, nq and the filter vary from call to call"""
    import torch
    kinds = cs.range_chain(index)
    assert len(kinds) >= 2 and len({cs.radii(k.name) for k in kinds}) == 1
    want = {k.name: isolated(k.name) for k in kinds}
    idx = open_handle(index)
    st = torch.cuda.Stream(_dev())
    try:
        idx.set_range_search(cs.radii(kinds[0].name)[0])
        for seed in (3451, 3452, 3453):
            seq = [kinds[i] for i in np.random.default_rng(seed).permutation(len(kinds))] * 2
            for k, got in zip(seq, run_chain(idx, st, seq)):
                same_bits(got, want[k.name], f"range chain: {k.name} in {[s.name for s in seq]}")
        idx.set_range_search(None)
        k = next(k for k in kinds_of(index) if cs.plain(k))
        same_bits(run(idx, k, st), isolated(k.name), f"{k.name} after the range chains")
    finally:
        idx.close()


# ---- 4. two streams, interleaved ---------------------------------------------------------------------------------------------------------
def test_two_streams_interleaved():
    import torch
    s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    c1, c2 = chains("A")[1][:14], chains("A")[2][:14]
    want = {k.name: isolated(k.name) for k in c1 + c2}
    idx = open_handle("A")
    try:
        for rnd in range(2):
            o1, o2 = [Pending(k, s1) for k in c1], [Pending(k, s2) for k in c2]
            for k in c1 + c2:
                dev_inputs(k)
            for (k1, a), (k2, b) in zip(zip(c1, o1), zip(c2, o2)):
                enqueue(idx, k1, s1, a)
                enqueue(idx, k2, s2, b)
            s1.synchronize()
            s2.synchronize()
            for k, o in list(zip(c1, o1)) + list(zip(c2, o2)):
                same_bits(o.result(), want[k.name], f"round {rnd}: {k.name} on two streams")
            idx.release_stream(s1.cuda_stream)  # the stream's workspace is freed; the next call on it starts a new one
    finally:
        idx.close()


# ---- 5. host entry: pool lanes, shrinking sub-batches, call_nq / latency_first put back -------------------------------------------------
HOST_SEQUENCE = ["a_host_nq8_sub3", "a_host_nq700_sub64", "a_nq200", "a_host_nq1", "a_nq5", "a_host_nq8_sub3"]


@pytest.mark.parametrize("replicas", [1, 2])
def test_host_entry(replicas):
    import torch
    idx = open_handle("A", **({"devices": [0, 0]} if replicas == 2 else {}))
    st = torch.cuda.Stream(_dev())
    try:
        assert idx.device_count() == replicas
        for name in HOST_SEQUENCE:
            same_bits(run(idx, BY_NAME[name], st), isolated(name), f"{name} in {HOST_SEQUENCE}, {replicas} replica(s)")
    finally:
        idx.close()


# ---- 6. a refused call in the middle ---------------------------------------------------------------------------------------------------
def _refusals(idx, stream):
    """[(what, kind of error, a word of its detail, the call)]: every call is refused before anything is launched; the output buffers are
    nevertheless as large as the call's would be"""
    import torch
    c = case("A")
    dim, L = c.q.shape[1], rq_index.lib()
    qh = np.ascontiguousarray(c.q[:2])
    qd = torch.from_numpy(qh).to(_dev())
    half = torch.zeros(2 * dim + 8, dtype=torch.float16, device=_dev())
    half_h = np.zeros(2 * dim + 8, np.float16)

    def device(qptr, nq, qdim, top_k):
        o = (torch.zeros((nq, top_k), dtype=torch.int64, device=_dev()), torch.zeros((nq, top_k), dtype=torch.float32, device=_dev()),
             torch.zeros(nq, dtype=torch.int32, device=_dev()))
        torch.cuda.synchronize(_dev())
        idx.search_batch_device(qptr, nq, qdim, top_k, 6, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream=C.c_void_p(stream.cuda_stream))

    def host(qptr, nq, qdim, top_k):
        ids, sc, cnt, _ = _host_buffers(nq, top_k, False)
        rq_index._check(L.rbq_search_batch(idx._h, qptr, nq, qdim, top_k, 6, None, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None))

    @contextlib.contextmanager
    def opts(*pairs, radius=None):
        try:
            for n, v, _ in pairs:
                idx.set_option(n, v)
            if radius is not None:
                idx.set_range_search(radius)
            yield
        finally:
            if radius is not None:
                idx.set_range_search(None)
            for n, _, back in reversed(pairs):
                idx.set_option(n, back)

    out = []
    for entry, call, q, q16 in (("device", device, qd.data_ptr(), half.data_ptr()), ("host", host, qh.ctypes.data, half_h.ctypes.data)):
        out += [
            (f"{entry}: a wrong query_dim", "DimensionMismatch", "expected", opts(), lambda call=call, q=q: call(q, 2, dim + 1, 10)),
            (f"{entry}: top_k above 2^20", "InvalidConfig", "top_k", opts(), lambda call=call, q=q: call(q, 1, dim, (1 << 20) + 1)),
            (f"{entry}: range search with the rerank on", "InvalidConfig", "range search", opts(("rerank", 1, 0), radius=np.float32(1.0)),
             lambda call=call, q=q: call(q, 2, dim, 10)),
            (f"{entry}: top_k 2000 with the rerank on", "InvalidConfig", "rerank", opts(("rerank", 1, 0)), lambda call=call, q=q: call(q, 2, dim, 2000)),
            (f"{entry}: a misaligned 16-bit query pointer", "InvalidConfig", "aligned", opts(("query_dtype", 1, 0)),
             lambda call=call, q16=q16: call(q16 + 1, 2, dim, 10)),
        ]
    return out, (qh, qd, half, half_h)  # (the second value keeps the buffers alive)


def test_refused_calls_in_the_middle():
    import torch
    idx = open_handle("A")
    st = torch.cuda.Stream(_dev())
    x, ys = BY_NAME["a_widest"], [(BY_NAME["a_nq200"], "device"), (BY_NAME["a_host_nq8_sub3"], "host"), (BY_NAME["a_nq4"], "device"),
                                   (BY_NAME["a_nq4"], "host")]
    try:
        refusals, keep = _refusals(idx, st)
        assert len(refusals) == 10
        for what, kind, word, ctx, call in refusals:
            run(idx, x, st)
            with ctx:
                with pytest.raises(rq.RabitqError, match=word) as e:
                    call()
            assert e.value.kind == kind and e.value.detail, what
            for y, entry in ys:
                same_bits(run(idx, y, st, entry), isolated(y.name), f"{y.name} ({entry} entry) after {what}")
        del keep
    finally:
        idx.close()


# ---- 8. fetch alongside search ----------------------------------------------------------------------------------------------------------
def test_fetch_between_searches():
    import torch
    ids = np.random.default_rng(3461).choice(len(case("A").data), 100, replace=False).astype(np.uint64)
    fresh = open_handle("A")
    try:
        want, found = fresh.fetch_embeddings(ids)
        assert found.all() and np.abs(want).sum() > 0
    finally:
        fresh.close()
    idx = open_handle("A")
    st = torch.cuda.Stream(_dev())
    try:
        for name in ("a_widest", "a_nq200", "a_host_nq8_sub3"):
            same_bits(run(idx, BY_NAME[name], st), isolated(name), f"{name} before the fetch")
            got, gfound = idx.fetch_embeddings(ids)
            assert gfound.all() and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"the fetch after {name} differs from a fresh handle's"
            same_bits(run(idx, BY_NAME[name], st), isolated(name), f"{name} after the fetch")
    finally:
        idx.close()
