"""rbq_index_remove_ids (include/rbq_remove.h): vectors removed from a device-resident index on the GPU.  The
yardstick is never the new code: the shrunk handle must equal, array for array and byte for byte, the index the existing one-shot
encoder (rbq_index_build_device_ex) builds over the rows that stay (its `ids` mapped back to the original ids); its saved bytes
must equal tests/rbq1_writer.py's over the CPU builder's clusters of those rows; its fetches tests/fetch_ref.py's.  Every
comparison is exact."""
import numpy as np
import pytest

import fetch_ref
import rabitq_rs_amd as rq
import rbq1_writer
from conftest import make_dataset
from test_gpu_append import ARRAYS, Case, _arrays

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_R69 = sorted(np.random.default_rng(2207).choice(100, 69, replace=False).tolist())
# geometry edges: (list size, positions removed, in in-list order — ascending id order for a one-shot build)
GEO = [
    (0, []),                          # nothing to remove
    (1, []),
    (1, [0]),                         # the list empties and later lists shift
    (5, [0]),                         # the first
    (5, [4]),                         # the last
    (31, []),
    (32, [7]),                        # a full block becomes partial
    (32, list(range(32))),            # the block disappears
    (33, [32]),                       # the tail block disappears
    (33, [0]),                        # every lane shifts across the block edge
    (64, list(range(0, 64, 2))),      # every second vector
    (64, list(range(32))),            # block 0 whole: block 1 becomes block 0 in identical lanes
    (100, [31, 32, 57]),              # lane 31 of block 0, lane 0 of block 1, one in the middle
    (100, _R69),                      # 69, leaving 31
    (100, list(range(100))),          # all
    (70, []),                         # a pure shift behind lists that shrank
]
SIZES = [s for s, _ in GEO]


def _geo_case(dim, bits, metric, rot, faster, seed):
    cs = Case(dim, bits, metric, rot, faster, SIZES, [0] * len(SIZES), seed)
    gone = np.concatenate([np.nonzero(cs.assign == c)[0][pos] for c, (_, pos) in enumerate(GEO) if pos]).astype(np.uint64)
    return cs, gone


def _kept(n, gone):
    """K: the rows whose id is not in the set, ascending"""
    keep = np.ones(n, bool)
    g = np.asarray(gone, np.uint64)
    keep[g[g < n].astype(np.int64)] = False
    return np.nonzero(keep)[0]


def _one_shot_rows(cs, K):
    """the existing encoder over rows X[K] with a[K]: ids 0 .. len(K) - 1"""
    import torch
    xk = cs.xd[torch.from_numpy(K).cuda()].contiguous()
    ak = torch.from_numpy(cs.assign[K].astype(np.int32)).cuda()
    return rq.IvfRabitqIndex.build_on_device(cs.built.hdr_ptr, cs.cent, xk.data_ptr(), ak.data_ptr(), len(K), cs.t, rescale=cs.rescale)


def _same_but_ids(ref, got, K, what=""):
    """every array of the contract; `ids` with every real slot's value j of `ref` replaced by K[j], pads all ones"""
    a, b = _arrays(ref), _arrays(got)
    for name in ARRAYS:
        assert a[name].size == b[name].size, (what, name, a[name].size, b[name].size)
        want = a[name]
        if name == "ids":
            j = want.view(np.uint64)
            want = np.where(j == ONES, ONES, np.asarray(K, np.uint64)[np.where(j == ONES, 0, j).astype(np.int64)]).view(np.uint8)
        bad = np.nonzero(want != b[name])[0]
        assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first at {bad[:5]}"
    assert len(ref) == len(got)


def _clusters(built, idmap):
    """the CPU builder's clusters as rbq1_writer takes them, ids mapped through idmap"""
    ex = int(built.header.ex_bits)
    out = []
    for c in range(int(built.header.n_lists)):
        a = built.list_arrays(c)
        n = len(a["ids"])
        out.append({"centroid": [float(v) for v in a["centroid"]], "ids": [int(idmap[int(i)]) for i in a["ids"]],
                    "batch_data": a["batch_data"].tobytes(), "ex_codes": [a["ex_codes"][v].tobytes() if ex else b"" for v in range(n)],
                    "f_add_ex": a["f_add_ex"].tolist(), "f_rescale_ex": a["f_rescale_ex"].tolist(), "delta": a["delta"].tolist(),
                    "vl": a["vl"].tolist()})
    return out


def _stream(built, clusters):
    h = built.header
    return rbq1_writer.write_rbq1(int(h.dim), int(h.padded_dim), int(h.metric), int(h.rotator), int(h.ex_bits), built.rotator_blob(),
                                  clusters)


def _writer_bytes_of_kept(cs, K, bits, metric, rot, seed):
    """rbq1_writer over the CPU builder's clusters of the kept rows, each cluster's ids mapped back to the original ids"""
    kept = rq.builder.train_with_clusters(cs.data[K], cs.cent, cs.assign[K], bits, metric, rot, seed + 2, cs.faster)
    blob = _stream(kept, _clusters(kept, K))
    kept.close()
    return blob


def _results(idx, q, top_k, nprobe):
    ids, sc, cnt, _ = idx.batch_search_raw(q, rq.SearchParams(top_k, nprobe))
    return ids, sc.tobytes(), np.asarray(cnt).astype(np.int64).tolist()


# ---- 1. geometry edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,bits,metric,rot,faster", [
    pytest.param(64, 7, 0, 1, True, id="d64_kac_7bit_L2_const_tail_only"),
    pytest.param(128, 3, 1, 1, False, id="d128_kac_3bit_IP_optimal_one_granule"),
    pytest.param(130, 7, 0, 1, True, id="d130_kac_7bit_granule_plus_tail"),
    pytest.param(48, 1, 0, 0, True, id="d48_matrix_1bit_no_ex"),
    pytest.param(960, 7, 0, 1, True, id="d960_kac_7bit_seven_granules_plus_tail"),
    pytest.param(2048, 7, 0, 1, True, id="d2048_kac_7bit_sixteen_granules"),
])
def test_remove_equals_one_shot_build_of_the_kept_rows_at_the_geometry_edges(dim, bits, metric, rot, faster):
    seed = 3100 + dim + bits
    cs, gone = _geo_case(dim, bits, metric, rot, faster, seed)
    K = _kept(cs.n, gone)
    want = _one_shot_rows(cs, K)
    idx = cs.one_shot()
    removed = idx.remove_ids(gone)
    assert removed == gone.size == cs.n - len(K)
    assert len(idx) == len(K) and idx.id_bound() == int(K.max()) + 1
    ln = idx.debug_copy_index("list_n", np.empty(cs.nl, np.uint32))
    assert ln.tolist() == [s - len(pos) for s, pos in GEO]
    _same_but_ids(want, idx, K, "remove")
    assert idx.save_to_bytes() == _writer_bytes_of_kept(cs, K, bits, metric, rot, seed), "saved bytes differ from the writer's"
    want.close(); idx.close()


# ---- 2. search ---------------------------------------------------------------------------------------------------------------
def test_search_equals_the_kept_rows_index_and_never_returns_a_removed_id():
    nl = 7
    rng = np.random.default_rng(3201)
    cs = Case(64, 7, 0, 1, True, rng.multinomial(150, np.ones(nl) / nl).tolist(), [0] * nl, 3202)
    gone = rng.choice(cs.n, 110, replace=False).astype(np.uint64)
    K = _kept(cs.n, gone)
    want = _one_shot_rows(cs, K)
    idx = cs.one_shot()
    assert idx.remove_ids(gone) == 110
    for top_k in (10, 64):  # 64 is above the 40 vectors that stay
        wi, ws, wc = _results(want, cs.q, top_k, nl)
        gi, gs, gc = _results(idx, cs.q, top_k, nl)
        mapped = np.where(wi == ONES, ONES, K.astype(np.uint64)[np.where(wi == ONES, 0, wi).astype(np.int64)])
        assert np.array_equal(gi, mapped) and gs == ws and gc == wc, top_k
        assert not np.isin(gi, gone).any()
    assert gc == [len(K)] * len(cs.q)  # every vector that stayed is returned at top_k = 64, nprobe = n_lists
    want.close(); idx.close()


# ---- 3. add then remove is the identity --------------------------------------------------------------------------------------
def test_add_then_remove_is_the_identity_and_removals_compose():
    import torch
    from test_gpu_append import ADD, OLD, _same_index
    cs = Case(64, 7, 0, 1, True, OLD, ADD, 3300)
    want = cs.one_shot(cs.n_old)
    idx = cs.one_shot(cs.n_old)
    idx.add(cs.xd[cs.n_old:], cs.ad[cs.n_old:], first_id=cs.n_old)
    assert len(idx) == cs.n
    assert idx.remove_ids(range(cs.n_old, cs.n)) == cs.n_add
    assert idx.id_bound() == cs.n_old
    _same_index(want, idx, "add then remove")  # every array, ids included, and the saved bytes
    want.close(); idx.close()

    # two removals in sequence equal one removal of the union
    rng = np.random.default_rng(3301)
    s1 = rng.choice(cs.n, 200, replace=False).astype(np.uint64)
    s2 = rng.choice(cs.n, 150, replace=False).astype(np.uint64)  # overlaps s1: those ids are gone already
    union = np.union1d(s1, s2)
    two, one = cs.one_shot(), cs.one_shot()
    r1 = two.remove_ids(s1)
    r2 = two.remove_ids(s2)
    assert r1 == 200 and r1 + r2 == union.size == one.remove_ids(union)
    _same_index(one, two, "two removals")

    # a host array, shuffled, with repeats and ids that are not stored, against a sorted CUDA tensor of the set
    messy = np.concatenate([union, union[::3], np.array([cs.n, cs.n + 5, 1 << 40, (1 << 64) - 1], np.uint64)])
    rng.shuffle(messy)
    host, dev = cs.one_shot(), cs.one_shot()
    assert host.remove_ids(messy) == union.size
    assert dev.remove_ids(torch.from_numpy(union.astype(np.int64)).cuda()) == union.size
    _same_index(one, host, "host ids")
    _same_index(one, dev, "device ids")
    # nothing matches: the result equals the index; an empty set is no call at all
    same = cs.one_shot()
    assert same.remove_ids([cs.n, cs.n + 1]) == 0 and same.remove_ids([]) == 0
    full = cs.one_shot()
    _same_index(full, same, "nothing matched")
    # a set that covers every vector is refused (rbq_index_build_device_ex refuses zero rows); the handle stays as it was
    with pytest.raises(rq.RabitqError) as e:
        same.remove_ids(np.arange(cs.n + 3))
    assert e.value.kind == "InvalidConfig" and "every vector" in str(e.value)
    _same_index(full, same, "after the refusal")
    for i in (two, one, host, dev, same, full):
        i.close()


# ---- 4. a loaded handle with duplicated ids ----------------------------------------------------------------------------------
def test_loaded_handle_loses_every_slot_of_a_duplicated_id():
    cs, _ = _geo_case(64, 7, 0, 1, True, 3400)
    idmap = 7 * np.arange(cs.n, dtype=np.uint64) + 3
    r1, r2 = int(np.nonzero(cs.assign == 6)[0][5]), int(np.nonzero(cs.assign == 12)[0][40])
    idmap[r2] = idmap[r1]  # one id stored in two lists
    lone = int(np.nonzero(cs.assign == 3)[0][2])
    idx = rq.IvfRabitqIndex.load_from_bytes(_stream(cs.built, _clusters(cs.built, idmap)))
    assert len(idx) == cs.n
    assert idx.remove_ids([int(idmap[r1]), int(idmap[lone]), 5]) == 3  # both slots of the duplicated id, one more, one not stored
    K = np.array([i for i in range(cs.n) if i not in (r1, r2, lone)])
    kept = rq.builder.train_with_clusters(cs.data[K], cs.cent, cs.assign[K], 7, 0, 1, 3402, True)
    want = _stream(kept, _clusters(kept, idmap[K]))
    assert len(idx) == cs.n - 3 and idx.save_to_bytes() == want
    assert idx.id_bound() == int(idmap[K].max()) + 1
    kept.close(); idx.close()


# ---- 5. fetch, and the old handle --------------------------------------------------------------------------------------------
def test_fetch_after_a_removal_and_the_old_handle_is_only_read():
    import ctypes as C
    from rabitq_rs_amd.index import _check, lib
    cs, gone = _geo_case(130, 7, 0, 1, True, 3500)
    K = _kept(cs.n, gone)
    old = cs.one_shot()
    every = np.arange(cs.n, dtype=np.uint64)
    emb0, found0 = old.fetch_embeddings(every)  # (builds the old handle's id map)
    assert found0.all()
    before = _results(old, cs.q, 10, cs.nl)
    h, removed = C.c_void_p(), C.c_uint64()
    _check(lib().rbq_index_remove_ids(old._h, gone.ctypes.data, gone.size, 1, None, C.byref(removed), C.byref(h)))
    new = rq.IvfRabitqIndex(h)
    assert removed.value == gone.size
    after = _results(old, cs.q, 10, cs.nl)  # the old handle answers as before the call
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    emb, found = new.fetch_embeddings(every)  # the new handle builds its own id map
    assert not found[gone.astype(np.int64)].any() and found[K].all()
    assert emb[K].tobytes() == emb0[K].tobytes() and not emb[gone.astype(np.int64)].view(np.uint32).any()
    want, wfound = fetch_ref.fetch(new.save_to_bytes(), every)  # and the reference over what the new handle saves agrees
    assert np.array_equal(found, wfound) and emb.tobytes() == want.tobytes()
    emb1, found1 = old.fetch_embeddings(every)
    assert found1.all() and emb1.tobytes() == emb0.tobytes()
    old.close(); new.close()


# ---- 6. two replicas ---------------------------------------------------------------------------------------------------------
def test_shrunk_handle_replicates_over_a_device_list():
    cs, gone = _geo_case(64, 3, 0, 1, True, 3650)
    one, two = cs.one_shot(), cs.one_shot()
    assert one.remove_ids(gone) == gone.size and one.device_count() == 1
    assert two.remove_ids(gone, devices=[0, 0]) == gone.size and two.device_count() == 2  # two replicas on one device
    q = make_dataset(64, 64, 4, 3653)
    a, b = _results(one, q, 10, cs.nl), _results(two, q, 10, cs.nl)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    two.set_option("debug_replica", 1)
    for name in ("blocks", "ids", "ex", "list_n", "bsumx"):
        assert _arrays(two)[name].tobytes() == _arrays(one)[name].tobytes(), name
    with pytest.raises(rq.RabitqError) as e:  # devices[0] must be the first replica's device
        one.remove_ids([1], devices=[99])
    assert e.value.kind == "InvalidConfig"
    one.close(); two.close()


def test_shrunk_handle_on_two_devices_searches_as_on_one():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    cs, gone = _geo_case(64, 3, 0, 1, True, 3600)
    one, two = cs.one_shot(), cs.one_shot()
    assert one.remove_ids(gone) == gone.size and one.device_count() == 1
    assert two.remove_ids(gone, devices=[0, 1]) == gone.size and two.device_count() == 2
    q = make_dataset(64, 64, 4, 3603)  # enough queries for both replicas to take a shard
    a, b = _results(one, q, 10, cs.nl), _results(two, q, 10, cs.nl)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    one.close(); two.close()


# ---- 7. argument errors on a live handle, in their order ---------------------------------------------------------------------
def test_argument_errors_come_in_the_documented_order_and_leave_the_handle_untouched():
    import ctypes as C
    from rabitq_rs_amd.index import _detail, lib
    cs, gone = _geo_case(64, 7, 0, 1, True, 3700)
    idx = cs.one_shot()
    bare = rq.IvfRabitqIndex.from_built_without_recon(cs.built)
    before = _results(idx, cs.q, 10, cs.nl)
    bad_dev = (C.c_int * 1)(99)

    def call(handle, ids, n, nd=1, dv=None):
        h, removed = C.c_void_p(0xDEAD), C.c_uint64(77)
        rc = lib().rbq_index_remove_ids(handle, ids, n, nd, dv, C.byref(removed), C.byref(h))
        assert rc == rq._abi.RBQ_INVALID_CONFIG and not h.value and removed.value == 77  # *out cleared, *out_removed untouched
        return _detail()

    assert "reconstruction" in call(bare._h, None, 0, 1, bad_dev)  # before null ids, n_ids == 0 and the device list
    assert call(idx._h, None, 0, 1, bad_dev) == "null ids"         # before n_ids == 0 and the device list
    assert call(idx._h, gone.ctypes.data, 0, 1, bad_dev) == "no ids"  # before the device list
    assert "device" in call(idx._h, gone.ctypes.data, gone.size, 1, bad_dev)
    assert "n_devices" in call(idx._h, gone.ctypes.data, gone.size, 17, (C.c_int * 17)(*([0] * 17)))
    after = _results(idx, cs.q, 10, cs.nl)
    assert len(idx) == cs.n and np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    idx.close(); bare.close()
