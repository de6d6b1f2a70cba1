"""rbq_index_append (include/rbq_append.h): vectors appended to a device-resident index on the GPU.  The
yardstick is never the new code: the appended handle must equal, array for array and byte for byte, the index the existing
one-shot encoder (rbq_index_build_device_ex) builds over the old and the new rows together; its saved bytes must equal the CPU
builder's; its search results the oracle's; the nearest-centroid assignment tests/kmeans_ref.py's.  Every comparison is exact."""
import ctypes as C
import re

import numpy as np
import pytest

import kmeans_ref
import rabitq_rs_amd as rq
import rbq1_writer
from conftest import make_dataset
from rabitq_rs_amd.index import _detail, lib
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

# the arrays of the contract
ARRAYS = ("list_gb0", "list_n", "centroids", "cnorm2", "cent_hl", "blocks", "ids", "ex", "fadd_ex", "fres_ex", "bsum", "bsumx", "lsum",
          "delta", "vl")
# geometry edges: empty stays empty, empty gets blocks, untouched partial, partial stays partial, partial fills exactly, partial
# overflows into new blocks, 31 + 1, full untouched, full opens a block, 33 + 31 ends on a block edge, multi-block untouched,
# multi-block grows; every later list is shifted
OLD = [0, 0, 1, 5, 5, 5, 31, 32, 32, 33, 64, 100]
ADD = [0, 40, 0, 3, 27, 60, 1, 0, 1, 31, 0, 70]


def _arrays(idx):
    """every array of the contract as bytes (the library says how long each is)"""
    out = {}
    for name in ARRAYS:
        rc = lib().rbq_debug_copy_index(idx._h, name.encode(), C.byref(C.c_uint8()), 0)
        n = 0 if rc == 0 else int(re.search(r"have (\d+) bytes", _detail()).group(1))
        buf = np.empty(n, np.uint8)
        if n:
            idx.debug_copy_index(name, buf)
        out[name] = buf
    return out


def _same_index(ref, got, what=""):
    a, b = _arrays(ref), _arrays(got)
    for name in ARRAYS:
        assert a[name].size == b[name].size, (what, name, a[name].size, b[name].size)
        bad = np.nonzero(a[name] != b[name])[0]
        assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first at {bad[:5]}"
    assert len(ref) == len(got)
    assert ref.save_to_bytes() == got.save_to_bytes(), f"{what}: saved bytes differ"


class Case:
    """old + new rows with their lists, centroids, the CPU builder's index over the union (header, t_const, oracle)"""

    def __init__(self, dim, bits, metric, rot, faster, old, add, seed, mult=1):
        import torch
        old, add = [s * mult for s in old], [s * mult for s in add]
        self.nl, self.n_old, self.n_add = len(old), sum(old), sum(add)
        self.n = self.n_old + self.n_add
        rng = np.random.default_rng(seed)
        self.data = make_dataset(self.n, dim, 4, seed + 1, normalize=(metric == 1))
        a_old = rng.permutation(np.repeat(np.arange(self.nl), old))
        a_new = rng.permutation(np.repeat(np.arange(self.nl), add))  # a seeded shuffle of the multiset
        self.assign = np.concatenate([a_old, a_new]).astype(np.uint32)
        self.cent = np.stack([self.data[self.assign == c].mean(0) if (self.assign == c).any() else self.data[c]
                              for c in range(self.nl)]).astype(np.float32)
        self.faster, self.rescale = faster, "const" if faster else "optimal"
        self.built = rq.builder.train_with_clusters(self.data, self.cent, self.assign, bits, metric, rot, seed + 2, faster)
        self.t = self.built.t_const if faster else None
        self.xd = torch.from_numpy(self.data).cuda()
        self.ad = torch.from_numpy(self.assign.astype(np.int32)).cuda()
        self.q = make_dataset(16, dim, 4, seed + 3, normalize=(metric == 1))

    def one_shot(self, n=None, assign=None):
        """the existing encoder over rows [0, n) (all by default)"""
        import torch
        n = self.n if n is None else n
        ad = self.ad if assign is None else torch.from_numpy(np.asarray(assign).astype(np.int32)).cuda()
        return rq.IvfRabitqIndex.build_on_device(self.built.hdr_ptr, self.cent, self.xd.data_ptr(), ad.data_ptr(), n, self.t,
                                                 rescale=self.rescale)


def _results(idx, q, nprobe):
    ids, sc, cnt, _ = idx.batch_search_raw(q, rq.SearchParams(10, nprobe))
    return ids.tobytes(), sc.tobytes(), cnt.tobytes()


# ---- 1. geometry edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,bits,metric,rot,faster,mult", [
    pytest.param(64, 7, 0, 1, True, 1, id="d64_kac_7bit_L2_const"),
    pytest.param(50, 3, 1, 1, False, 1, id="d50_pad64_kac_3bit_IP_optimal"),
    pytest.param(48, 1, 0, 0, True, 1, id="d48_matrix_1bit_L2"),
    pytest.param(128, 7, 0, 1, False, 1, id="d128_kac_7bit_L2_optimal"),
    pytest.param(960, 7, 0, 1, True, 3, id="d960_kac_7bit_L2_const_x3"),
])
def test_append_equals_one_shot_build_at_the_geometry_edges(dim, bits, metric, rot, faster, mult):
    cs = Case(dim, bits, metric, rot, faster, OLD, ADD, 2100 + dim + bits, mult)
    want = cs.one_shot()
    idx = cs.one_shot(cs.n_old)
    assert idx.id_bound() == cs.n_old
    got = idx.add(cs.xd[cs.n_old:], cs.ad[cs.n_old:], first_id=cs.n_old)
    assert np.array_equal(got, cs.assign[cs.n_old:])
    assert len(idx) == cs.n and idx.id_bound() == cs.n
    _same_index(want, idx, "append")
    _compare(cs.built, idx, cs.q, 10, cs.nl)
    want.close(); idx.close()


# ---- 2. chunked and repeated appends -----------------------------------------------------------------------------------------
def test_three_appends_chunked_host_and_device_equal_one_build():
    nl = 9
    rng = np.random.default_rng(2201)
    old = rng.multinomial(300, np.ones(nl) / nl).tolist()
    cs = Case(64, 7, 0, 1, True, old, rng.multinomial(938, np.ones(nl) / nl).tolist(), 2202)
    want = cs.one_shot()
    idx = cs.one_shot(cs.n_old)
    cuts = [cs.n_old, cs.n_old + 237, cs.n_old + 238, cs.n]
    for k, (a, b, cap) in enumerate(zip(cuts[:-1], cuts[1:], (64, 0, 64))):
        p0 = lib().rbq_debug_append_passes()
        if k % 2 == 0:  # host pointers
            got = idx.add(cs.data[a:b], cs.assign[a:b], max_chunk_rows=cap)
        else:           # device pointers
            got = idx.add(cs.xd[a:b], cs.ad[a:b], first_id=a, max_chunk_rows=cap)
        assert np.array_equal(got, cs.assign[a:b])
        passes = lib().rbq_debug_append_passes() - p0
        assert passes == ((b - a + 63) // 64 if cap else 1), (k, passes)  # 237 rows in chunks of 64: 4 encode passes
    _same_index(want, idx, "three appends")
    # the cap is rounded up to a multiple of 64: 65 -> 128 rows per pass
    idx2 = cs.one_shot(cs.n_old)
    p0 = lib().rbq_debug_append_passes()
    idx2.add(cs.data[cs.n_old:], cs.assign[cs.n_old:], max_chunk_rows=65)
    assert lib().rbq_debug_append_passes() - p0 == (cs.n_add + 127) // 128
    _same_index(want, idx2, "cap 65")
    want.close(); idx.close(); idx2.close()


# ---- 3. nearest-centroid assignment ------------------------------------------------------------------------------------------
def _nearest_case(nl, dim, seed):
    rng = np.random.default_rng(seed)
    n_old, n_add = 3 * nl, 260
    cs = Case.__new__(Case)
    import torch
    data = make_dataset(n_old + n_add, dim, 4, seed + 1)
    cent = data[rng.choice(n_old, nl, replace=False)].copy()
    cent[5] = cent[2]                      # two identical centroids: the lower index wins
    if nl >= 300:
        cent[20:290] = cent[20]            # 270 identical centroids: more exact ties than a shortlist holds (256)
        data[n_old + 4:n_old + 24] = cent[20] + 0.01 * rng.standard_normal((20, dim)).astype(np.float32)
    data[n_old] = cent[3]                  # a row equal to a centroid
    data[n_old + 1] = cent[2]              # a row equal to the duplicated centroid
    data[n_old + 2] = cent[2] + np.float32(1e-3)
    a_old = rng.integers(0, nl, n_old).astype(np.uint32)
    cs.nl, cs.n_old, cs.n_add, cs.n = nl, n_old, n_add, n_old + n_add
    cs.data, cs.cent, cs.assign = data, cent, np.concatenate([a_old, np.zeros(n_add, np.uint32)])
    cs.faster, cs.rescale = True, "const"
    cs.built = rq.builder.train_with_clusters(data[:n_old], cent, a_old, 7, 0, 1, seed + 2, True)
    cs.t = cs.built.t_const
    cs.xd = torch.from_numpy(data).cuda()
    cs.ad = torch.from_numpy(cs.assign.astype(np.int32)).cuda()
    cs.q = make_dataset(16, dim, 4, seed + 3)
    return cs


@pytest.mark.parametrize("nl,dim", [pytest.param(7, 64, id="7_lists_d64"), pytest.param(300, 128, id="300_lists_d128")])
def test_nearest_centroid_assignment_matches_the_restatement(nl, dim):
    cs = _nearest_case(nl, dim, 2300 + nl)
    idx = cs.one_shot(cs.n_old)
    D = idx.padded_dim
    crot = idx.debug_copy_index("centroids", np.empty((nl, D), np.float32))
    xnew = cs.data[cs.n_old:]
    xrot = np.stack([cs.built.rotate(x) for x in xnew])
    want, _ = kmeans_ref.assign(xrot, kmeans_ref.norms(xrot), crot)
    assert want[1] == 2 and 5 not in want and (nl < 300 or ((want[4:24] == 20).all() and not ((want > 20) & (want < 290)).any()))
    before = _results(idx, cs.q, nl)
    bad = xnew.copy()
    bad[77, 3] = np.nan
    with pytest.raises(rq.RabitqError) as e:  # a NaN row is refused; the handle still answers as before
        idx.add(bad)
    assert e.value.kind == "InvalidConfig" and "non-finite" in str(e.value)
    assert len(idx) == cs.n_old and _results(idx, cs.q, nl) == before
    got = idx.add(cs.xd[cs.n_old:], max_chunk_rows=128)  # returned lists
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    # stored lists: the new ids sit in the lists the restatement names
    ln = idx.debug_copy_index("list_n", np.empty(nl, np.uint32))
    assert np.array_equal(ln, np.bincount(cs.assign[:cs.n_old], minlength=nl) + np.bincount(want, minlength=nl))
    # the same index as an append with that assignment given, from host rows, and as the one-shot build
    idx2 = cs.one_shot(cs.n_old)
    got2 = idx2.add(xnew, want)
    assert np.array_equal(got2, want)
    _same_index(idx2, idx, "explicit vs nearest")
    one = cs.one_shot(assign=np.concatenate([cs.assign[:cs.n_old], want]))
    _same_index(one, idx, "one-shot vs nearest")
    idx.close(); idx2.close(); one.close()


# ---- 4. a loaded handle ------------------------------------------------------------------------------------------------------
def test_append_to_a_loaded_handle_saves_the_cpu_builders_bytes():
    cs = Case(64, 7, 0, 1, True, OLD, ADD, 2400)
    old = rq.builder.train_with_clusters(cs.data[:cs.n_old], cs.cent, cs.assign[:cs.n_old], 7, 0, 1, 2402, True)
    idx = rq.IvfRabitqIndex.load_from_bytes(old.save_rbq1())
    with pytest.raises(rq.RabitqError) as e:  # a loaded object does not know its rescale mode
        idx.add(cs.data[cs.n_old:], cs.assign[cs.n_old:])
    assert e.value.kind == "InvalidConfig" and "rescale" in str(e.value) and "t_const" in str(e.value)
    idx.add(cs.data[cs.n_old:], cs.assign[cs.n_old:], rescale="const", t_const=cs.built.t_const)
    assert idx.save_to_bytes() == cs.built.save_rbq1()
    one = cs.one_shot()
    new_ids = np.arange(cs.n_old, cs.n, dtype=np.uint64)
    a, fa = idx.fetch_embeddings(new_ids)
    b, fb = one.fetch_embeddings(new_ids)
    assert fa.all() and fb.all() and a.tobytes() == b.tobytes()
    words = np.zeros((cs.n + 31) // 32, np.uint32)  # search_filtered restricted to the new ids
    np.bitwise_or.at(words, (new_ids >> np.uint64(5)).astype(np.int64), np.uint32(1) << (new_ids & np.uint64(31)).astype(np.uint32))
    ids, _, cnt = _compare(cs.built, idx, cs.q, 10, cs.nl, words, cs.n)
    assert (cnt > 0).all() and (ids[ids != np.iinfo(np.uint64).max] >= cs.n_old).all()
    idx.close(); one.close(); old.close()


# ---- 5. replicas -------------------------------------------------------------------------------------------------------------
def test_append_replicates_like_the_streamed_builder():
    cs = Case(64, 3, 0, 1, True, OLD, ADD, 2500)
    old = rq.builder.train_with_clusters(cs.data[:cs.n_old], cs.cent, cs.assign[:cs.n_old], 3, 0, 1, 2502, True)
    two = rq.IvfRabitqIndex.from_built(old, devices=[0, 0])
    assert two.device_count() == 2
    two.add(cs.data[cs.n_old:], cs.assign[cs.n_old:], rescale="const", t_const=cs.built.t_const, devices=[0, 0])
    assert two.device_count() == 2 and len(two) == cs.n
    one = rq.IvfRabitqIndex.from_built(old)
    one.add(cs.data[cs.n_old:], cs.assign[cs.n_old:], rescale="const", t_const=cs.built.t_const)
    assert one.device_count() == 1
    q = make_dataset(64, 64, 4, 2503)  # enough queries for both replicas to take a shard
    assert _results(two, q, cs.nl) == _results(one, q, cs.nl)
    two.set_option("debug_replica", 1)
    for name in ("blocks", "ids", "ex", "list_n", "bsumx"):
        assert _arrays(two)[name].tobytes() == _arrays(one)[name].tobytes(), name
    with pytest.raises(rq.RabitqError) as e:  # devices[0] must be the first replica's device
        one.add(cs.data[:1], cs.assign[:1], devices=[99])
    assert e.value.kind == "InvalidConfig"
    two.close(); one.close(); old.close()


# ---- 6. errors found on the device, and the accessor -------------------------------------------------------------------------
def test_device_side_errors_leave_the_old_handle_untouched():
    cs = Case(64, 7, 0, 1, True, OLD, ADD, 2600)
    idx = cs.one_shot(cs.n_old)
    before = _results(idx, cs.q, cs.nl)
    arrays = {k: v.tobytes() for k, v in _arrays(idx).items()}
    new_x, new_a = cs.data[cs.n_old:], cs.assign[cs.n_old:]
    with pytest.raises(rq.RabitqError) as e:
        idx.add(new_x, new_a, first_id=cs.n_old - 1)
    assert e.value.kind == "InvalidConfig" and "id bound" in str(e.value)
    assert _results(idx, cs.q, cs.nl) == before
    bad = new_a.copy()
    bad[-1] = cs.nl
    for a in (bad, cs.ad.new_tensor(bad.astype(np.int32))):  # host and device assignments
        with pytest.raises(rq.RabitqError) as e:
            idx.add(new_x, a)
        assert e.value.kind == "InvalidConfig" and "out of range" in str(e.value)
        assert _results(idx, cs.q, cs.nl) == before
    for kw in (dict(rescale="best"), dict(rescale="const", t_const=0.0)):  # and two of the argument errors, on a live handle
        with pytest.raises(rq.RabitqError) as e:
            idx.add(new_x, new_a, **kw)
        assert e.value.kind == "InvalidConfig"
    with pytest.raises(rq.RabitqError) as e:
        idx.add(new_x[:0], new_a[:0])
    assert e.value.kind == "InvalidConfig" and str(e.value).endswith("no vectors")
    assert len(idx) == cs.n_old and idx.id_bound() == cs.n_old
    assert {k: v.tobytes() for k, v in _arrays(idx).items()} == arrays and _results(idx, cs.q, cs.nl) == before
    # a handle without reconstruction factors could not be saved afterwards
    old = rq.builder.train_with_clusters(cs.data[:cs.n_old], cs.cent, cs.assign[:cs.n_old], 7, 0, 1, 2602, True)
    bare = rq.IvfRabitqIndex.from_built_without_recon(old)
    with pytest.raises(rq.RabitqError) as e:
        bare.add(new_x, new_a, rescale="const", t_const=cs.built.t_const)
    assert e.value.kind == "InvalidConfig" and "reconstruction" in str(e.value)
    idx.close(); bare.close(); old.close()


def test_id_bound_of_built_and_sparse_loaded_handles():
    cs = Case(64, 3, 0, 1, True, OLD, ADD, 2700)
    idx = cs.one_shot()
    assert idx.id_bound() == cs.n and idx.id_bound() == cs.n  # (the second call is served from the handle)
    idx.close()
    h = cs.built.header
    clusters = []
    for c in range(cs.nl):  # the same index with sparse ids 7 i + 3, written by the independent writer
        a = cs.built.list_arrays(c)
        n = len(a["ids"])
        clusters.append({"centroid": a["centroid"].tolist(), "ids": [7 * int(i) + 3 for i in a["ids"]], "batch_data": a["batch_data"].tobytes(),
                         "ex_codes": [a["ex_codes"][v].tobytes() for v in range(n)], "f_add_ex": a["f_add_ex"].tolist(),
                         "f_rescale_ex": a["f_rescale_ex"].tolist(), "delta": a["delta"].tolist(), "vl": a["vl"].tolist()})
    blob = rbq1_writer.write_rbq1(int(h.dim), int(h.padded_dim), int(h.metric), int(h.rotator), int(h.ex_bits), cs.built.rotator_blob(),
                                  clusters)
    sparse = rq.IvfRabitqIndex.load_from_bytes(blob)
    assert sparse.id_bound() == 7 * (cs.n - 1) + 3 + 1
    with pytest.raises(rq.RabitqError):
        sparse.add(cs.data[:2], cs.assign[:2], first_id=7 * (cs.n - 1) + 3, rescale="const", t_const=cs.built.t_const)
    got = sparse.add(cs.data[:2], cs.assign[:2], rescale="const", t_const=cs.built.t_const)  # first_id defaults to the bound
    assert np.array_equal(got, cs.assign[:2]) and sparse.id_bound() == 7 * (cs.n - 1) + 3 + 3 and len(sparse) == cs.n + 2
    emb, found = sparse.fetch_embeddings([7 * (cs.n - 1) + 4, 7 * (cs.n - 1) + 5, 7 * (cs.n - 1) + 6])
    assert found.tolist() == [True, True, False]
    sparse.close()


# ---- 7. Python add -----------------------------------------------------------------------------------------------------------
def test_python_add_twice_equals_the_one_shot_object():
    n0, n1, n2, dim, nl = 900, 257, 400, 96, 12
    data = make_dataset(n0 + n1 + n2, dim, 4, 2801)
    cent, a0 = rq.builder.kmeans(data[:n0], nl, 4, 2802)
    idx = rq.IvfRabitqIndex.train_on_device(data[:n0], cent, a0, 7, 0, 1, 2803, True)
    g1 = idx.add(data[n0:n0 + n1])
    assert len(idx) == n0 + n1
    import torch
    g2 = idx.add(torch.from_numpy(data[n0 + n1:]).cuda())
    assert len(idx) == n0 + n1 + n2 and idx.id_bound() == len(idx)
    one = rq.IvfRabitqIndex.train_on_device(data, cent, np.concatenate([a0, g1, g2]), 7, 0, 1, 2803, True)
    assert len(one) == len(idx) and one.save_to_bytes() == idx.save_to_bytes()
    q = make_dataset(16, dim, 4, 2804)
    for a, b in zip(idx.batch_query(q, 10, nl), one.batch_query(q, 10, nl)):
        assert a.tobytes() == b.tobytes()
    _same_index(one, idx, "python add")
    # the numeric variant travels with the handle
    idx.set_numeric_variant("portable")
    idx.add(data[:3], first_id=10 ** 9)
    assert idx.numeric_variant == "portable" and idx.id_bound() == 10 ** 9 + 3
    idx.close(); one.close()
