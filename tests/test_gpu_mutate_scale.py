"""rbq_index_append and rbq_index_remove_ids (DESIGN.md sections 21 and 22) where tests/test_gpu_append.py and
tests/test_gpu_remove.py do not reach: an index wide enough that every grid-stride loop of k_append_carry, k_append_id_bound,
k_remove_mark, k_remove_slot_map and k_remove_gather takes a second pass; stored ids that use all 64 bits; removal sets far larger
than the index; sequences of removals and appends against a model of the live rows; the old handle serving beside a mutation.
The yardsticks are those of the two modules: the one-shot encoder (rbq_index_build_device_ex) over the same rows, array for array
and byte for byte, tests/rbq1_writer.py over the CPU builder's clusters for saved bytes, and numpy.  Never a second run of the
code under test, and every comparison is exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd.index import _check, _rescale, lib
from test_gpu_append import ADD, OLD, Case, _arrays, _same_index
from test_gpu_remove import ONES, _clusters, _geo_case, _kept, _one_shot_rows, _results, _same_but_ids, _stream

pytestmark = pytest.mark.gpu

U64 = np.uint64
# the lanes the launchers start at most (k_append.hip, k_remove.hip): a loop takes a second pass only above these
ID_BOUND_LANES = 2048 * 256
MARK_LANES = 8192 * 256
# A list of one vector still occupies a block of 32 slots.  k_remove_mark and k_remove_slot_map need more than 8192 x 256 + 64
# slots, 65 539 blocks; about 1 % of the lists below are empty and about 1 % span two blocks, so 66 000 lists give about 65 970
# blocks.  That is above every other threshold too (2 048 x 256 slots; 2 x 8 x CUs + 1 blocks for any part below 2 000 CUs); the
# tests assert all of them on the device they run on.
NL_WIDE = 66_000


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _blocks(list_n):
    return int(((np.asarray(list_n, np.int64) + 31) // 32).sum())


def _map_ids(ids, K):
    """result ids j of an index over rows K, as the ids K[j]; unfilled slots stay all ones"""
    return np.where(ids == ONES, ONES, np.asarray(K, U64)[np.where(ids == ONES, 0, ids).astype(np.int64)])


def _same_results(want, got, q, K=None, nprobe=64, what=""):
    """a 16-query search, top_k 10: ids (those of `want` mapped through K), scores and counts bit for bit"""
    wi, ws, wc = _results(want, q, 10, nprobe)
    gi, gs, gc = _results(got, q, 10, nprobe)
    if K is not None:
        wi = _map_ids(wi, K)
    assert np.array_equal(gi, wi) and gs == ws and gc == wc, what


def _real_ids(idx):
    """the ids of every real slot, sorted"""
    ids = _arrays(idx)["ids"].view(U64)
    return np.sort(ids[ids != ONES])


# ---- A. the wide index -------------------------------------------------------------------------------------------------------
def _wide_sizes(nl=NL_WIDE):
    s = np.ones(nl, np.int64)
    s[50::101] = 33                                    # two blocks with a one-lane tail
    s[40::97] = 0
    s[[7, 1003, 30011, nl - 9]] = [64, 100, 64, 100]   # a handful of longer lists
    assert s[0] == 1 and s[nl - 1] == 1
    return s


def _wide_case(bits, seed):
    """~87 000 rows at dim 64 (FHT-Kac, L2, constant rescale) in 66 000 lists; the rows go to the lists by a seeded shuffle.  The
    centroids are no means (the encoders accept any clustering): a list's centroid is its first row, so that searches find
    populated lists.  The CPU builder gives the header and t_const only: they depend on (dim, bits, seed) alone."""
    import torch
    sizes = _wide_sizes()
    nl, n = len(sizes), int(sizes.sum())
    rng = np.random.default_rng(seed)
    cs = Case.__new__(Case)
    cs.nl, cs.n, cs.n_old = nl, n, int(0.6 * n)
    cs.n_add = n - cs.n_old
    cs.sizes = sizes
    centers = rng.standard_normal((64, 64)).astype(np.float32)
    cs.data = (centers[rng.integers(0, 64, n)] + 0.35 * rng.standard_normal((n, 64))).astype(np.float32)
    cs.assign = rng.permutation(np.repeat(np.arange(nl), sizes)).astype(np.uint32)
    cs.order = np.argsort(cs.assign, kind="stable")  # rows by list, ascending id inside a list
    cs.start = np.concatenate([[0], np.cumsum(sizes)])
    cs.cent = rng.standard_normal((nl, 64)).astype(np.float32)
    cs.cent[sizes > 0] = cs.data[cs.order[cs.start[:-1][sizes > 0]]]
    cs.faster, cs.rescale = True, "const"
    cs.built = rq.builder.train_with_clusters(cs.data[:nl], cs.cent, np.arange(nl, dtype=np.uint32), bits, 0, 1, seed + 2, True)
    cs.t = cs.built.t_const
    cs.xd = torch.from_numpy(cs.data).cuda()
    cs.ad = torch.from_numpy(cs.assign.astype(np.int32)).cuda()
    cs.q = (cs.data[rng.choice(n, 16, replace=False)] + 0.05 * rng.standard_normal((16, 64))).astype(np.float32)
    return cs


def _rows_of(cs, c):
    return cs.order[cs.start[c]:cs.start[c + 1]]


@pytest.fixture(scope="module")
def wide():
    """the 3-bit wide case and the one-shot handle over all its rows (a reference: no test changes it)"""
    cs = _wide_case(3, 4100)
    full = cs.one_shot()
    yield cs, full
    full.close()


def _wide_gone(cs):
    """a seeded 40 % of the ids, every vector of lists 20 000 .. 23 999 (thousands of lists empty, every later list shifts by
    thousands of blocks), and both vectors at the block edge of every second 33-list"""
    rng = np.random.default_rng(4101)
    two = np.nonzero(cs.sizes == 33)[0][::2]
    edge = np.concatenate([_rows_of(cs, c)[31:33] for c in two])
    gone = np.union1d(np.union1d(rng.choice(cs.n, int(0.4 * cs.n), replace=False), cs.order[cs.start[20000]:cs.start[24000]]), edge)
    return gone.astype(U64)


def _append_wide(cs):
    """one-shot over the first 60 % of the rows, the rest appended in one call with explicit lists"""
    new_blocks, slots = _blocks(cs.sizes), _blocks(cs.sizes) * 32
    assert new_blocks > 2 * 8 * _cus() + 1, (new_blocks, _cus())  # every workgroup of the carry takes two blocks, some three
    assert slots > ID_BOUND_LANES
    idx = cs.one_shot(cs.n_old)
    assert idx.id_bound() == cs.n_old  # the reduction over the old handle, in more than one pass too
    assert _blocks(np.bincount(cs.assign[:cs.n_old], minlength=cs.nl)) * 32 > ID_BOUND_LANES
    got = idx.add(cs.xd[cs.n_old:], cs.ad[cs.n_old:], first_id=cs.n_old)
    assert np.array_equal(got, cs.assign[cs.n_old:])
    return idx


@pytest.mark.parametrize("bits", [pytest.param(3, id="3bit"), pytest.param(1, id="1bit_no_ex")])
def test_wide_append_equals_the_one_shot_build(bits, wide):
    if bits == 3:
        cs, want = wide
    else:  # no ex codes: the carry's null fadd_ex / fres_ex branch
        cs = _wide_case(1, 4110)
        want = cs.one_shot()
    idx = _append_wide(cs)
    assert len(idx) == cs.n and idx.id_bound() == cs.n
    assert _arrays(want)["ids"].size == _blocks(cs.sizes) * 32 * 8
    _same_index(want, idx, "wide append")
    idx.close()
    if bits != 3:
        want.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_wide_remove_equals_the_one_shot_build_of_the_kept_rows(where, wide):
    import torch
    cs, _ = wide
    gone = _wide_gone(cs)
    K = _kept(cs.n, gone)
    old_slots = _blocks(cs.sizes) * 32
    assert old_slots > MARK_LANES + 64, old_slots  # the mark and the slot map: a second pass that is more than one wave long
    kept_n = np.bincount(cs.assign[K], minlength=cs.nl)
    assert _blocks(kept_n) > 2 * 8 * _cus() + 1, (_blocks(kept_n), _cus())  # every workgroup of the gather takes two blocks
    assert (kept_n[20000:24000] == 0).all() and (kept_n[np.nonzero(cs.sizes == 33)[0][::2]] <= 31).all()
    want = _one_shot_rows(cs, K)
    idx = cs.one_shot()
    s = np.random.default_rng(4102).permutation(gone)
    removed = idx.remove_ids(s if where == "host" else torch.from_numpy(s.view(np.int64)).cuda())
    assert removed == gone.size == cs.n - len(K) and len(idx) == len(K)
    ln = idx.debug_copy_index("list_n", np.empty(cs.nl, np.uint32))
    assert np.array_equal(ln, kept_n)
    _same_but_ids(want, idx, K, "wide remove")
    assert idx.id_bound() == int(K.max()) + 1
    want.close(); idx.close()


def _with_row_in_list(assign, row, c):
    """the same multiset of lists, with `row` in list c: it swaps lists with the first row of c"""
    a = assign.copy()
    other = int(np.nonzero(a == c)[0][0])
    a[other], a[row] = a[row], a[other]
    return a


def test_wide_id_bound_reaches_the_first_and_the_last_pass(wide):
    cs, _ = wide
    n, last = cs.n, cs.nl - 1
    assert _blocks(cs.sizes) * 32 > ID_BOUND_LANES
    # the largest id in the last list (only the last pass of the reduction reaches it), id n - 5 in list 0
    a_last = _with_row_in_list(_with_row_in_list(cs.assign, n - 1, last), n - 5, 0)
    assert a_last[n - 1] == last and a_last[n - 5] == 0
    a_first = _with_row_in_list(cs.assign, n - 1, 0)  # the largest id in list 0, which the first pass reaches
    h_last, h_first = cs.one_shot(assign=a_last), cs.one_shot(assign=a_first)
    assert h_last.id_bound() == n and h_first.id_bound() == n
    # a removal does not inherit the bound: the reduction runs again over the shrunk index
    assert h_first.remove_ids(np.array([n - 1], U64)) == 1 and h_first.id_bound() == n - 1
    assert h_last.remove_ids(np.arange(n - 3, n, dtype=U64)) == 3 and h_last.id_bound() == n - 3
    assert h_last.remove_ids(np.array([n - 4], U64)) == 1 and h_last.id_bound() == n - 4  # n - 5 stayed, in list 0
    assert np.array_equal(_real_ids(h_last), np.arange(n - 4, dtype=U64))
    h_last.close(); h_first.close()


def test_wide_search_after_append_and_after_remove_equals_the_one_shot_handles(wide):
    cs, full = wide
    grown = _append_wide(cs)
    _same_results(full, grown, cs.q, what="appended")
    gone = _wide_gone(cs)
    K = _kept(cs.n, gone)
    want = _one_shot_rows(cs, K)
    assert grown.remove_ids(gone) == gone.size  # the shrunk handle of the appended one
    _same_results(want, grown, cs.q, K, what="shrunk")
    assert max(_results(want, cs.q, 10, 64)[2]) == 10  # (the queries do find vectors)
    want.close(); grown.close()


# ---- B. ids that use all 64 bits ---------------------------------------------------------------------------------------------
def _ids64(cs):
    """an id for every row of the geometry-edge case (list sizes SIZES of test_gpu_remove.py), and the pairs among them whose
    members agree in their low 32 bits"""
    rows = lambda c: np.nonzero(cs.assign == c)[0]  # noqa: E731
    ids = [3 * i + 10 for i in range(cs.n)]  # ordinary small ids
    pairs = []
    for k in range(6):   # x and x + 2^32, in different lists
        a, b = int(rows(5)[k]), int(rows(15)[k])
        ids[b] = ids[a] + 2 ** 32
        pairs.append((a, b))
    for k in range(6):   # x and x | 2^63
        a, b = int(rows(6)[k]), int(rows(10)[k])
        ids[b] = ids[a] | 2 ** 63
        pairs.append((a, b))
    same = [(int(rows(12)[2 * k]), int(rows(12)[2 * k + 1])) for k in range(5)] + [(int(rows(8)[31]), int(rows(8)[32]))]
    for a, b in same:    # x and x + 2^33 in the SAME list (one pair across a block edge)
        ids[b] = ids[a] + 2 ** 33
        pairs.append((a, b))
    for k, r in enumerate(rows(13)[10:20]):  # a run at and above 2^63
        ids[int(r)] = 2 ** 63 + k
    top = int(rows(14)[-1])
    ids[top] = 2 ** 64 - 2  # the largest id that can be stored: 2^64 - 1 marks a pad
    assert len(set(ids)) == cs.n
    return np.array(ids, dtype=U64), pairs, top


def _writer_bytes(cs, K, idmap, bits, metric, rot, seed):
    """rbq1_writer over the CPU builder's clusters of rows K (the seed is the Case's), their ids idmap[K]"""
    kept = rq.builder.train_with_clusters(cs.data[K], cs.cent, cs.assign[K], bits, metric, rot, seed + 2, cs.faster)
    blob = _stream(kept, _clusters(kept, np.asarray(idmap, U64)[K]))
    kept.close()
    return blob


@pytest.fixture(scope="module")
def geo64():
    cs, _ = _geo_case(64, 7, 0, 1, True, 4200)
    idmap, pairs, top = _ids64(cs)
    return cs, idmap, pairs, top, _stream(cs.built, _clusters(cs.built, idmap))


@pytest.mark.parametrize("where", ["host", "device"])
def test_remove_tells_ids_apart_that_agree_in_their_low_32_bits(where, geo64):
    import torch
    cs, idmap, pairs, top, blob = geo64
    idx = rq.IvfRabitqIndex.load_from_bytes(blob)
    assert len(idx) == cs.n and idx.id_bound() == 2 ** 64 - 1  # 2^64 - 2 is stored: id + 1
    go = [a if k % 2 == 0 else b for k, (a, b) in enumerate(pairs)]       # one member of every pair: the low or the high one
    stay = [b if k % 2 == 0 else a for k, (a, b) in enumerate(pairs)]
    go += [int(r) for r in np.nonzero(cs.assign == 13)[0][10:12]]         # two of the run above 2^63
    go += [int(r) for r in np.nonzero(cs.assign == 3)[0][:2]]             # and two ordinary ones
    go = np.array(sorted(set(go)))
    decoys = np.concatenate([idmap[stay] ^ U64(1 << 34), idmap[stay] ^ U64(1 << 62), np.array([5, 2 ** 63 + 5000, 2 ** 64 - 3, ONES], U64)])
    assert not np.isin(decoys, idmap).any()
    # unsorted, values below and above 2^63 mixed, repeats: a signed sort would put the values above 2^63 first and the binary
    # search would miss them
    s = np.random.default_rng(4201).permutation(np.concatenate([idmap[go], decoys, idmap[go][::2]]))
    assert (s >> U64(63)).any() and not (s >> U64(63)).all() and (np.diff(s.view(np.int64)) < 0).any()
    removed = idx.remove_ids(s if where == "host" else torch.from_numpy(s.view(np.int64)).cuda())
    K = _kept(cs.n, go)
    assert removed == go.size and len(idx) == cs.n - go.size == len(K)
    stored = _real_ids(idx)
    assert np.isin(idmap[stay], stored).all() and not np.isin(idmap[go], stored).any()  # every twin stays
    assert np.array_equal(stored, np.sort(idmap[K]))
    assert idx.id_bound() == 2 ** 64 - 1
    assert idx.save_to_bytes() == _writer_bytes(cs, K, idmap, 7, 0, 1, 4200), "saved bytes differ from the writer's"
    want = _one_shot_rows(cs, K)
    _same_results(want, idx, cs.q, idmap[K], nprobe=cs.nl, what="after the removal")
    want.close()
    # without 2^64 - 2 the bound is 1 + the next largest id
    assert idx.remove_ids([5, 2 ** 64 - 2, 2 ** 63 + 5000]) == 1  # (a Python list of ints below and above 2^63 keeps every bit)
    K = K[K != top]
    assert idx.id_bound() == int(idmap[K].max()) + 1 and idx.id_bound() > 2 ** 63
    assert idx.save_to_bytes() == _writer_bytes(cs, K, idmap, 7, 0, 1, 4200), "saved bytes differ from the writer's (second removal)"
    idx.close()


def test_a_set_that_agrees_only_in_the_low_32_bits_removes_nothing(geo64):
    cs, idmap, _, _, blob = geo64
    idx = rq.IvfRabitqIndex.load_from_bytes(blob)
    s = np.concatenate([idmap ^ U64(1 << 32), idmap ^ U64(1 << 63), idmap ^ U64(1 << 40), idmap + U64(1 << 33)])
    s = s[~np.isin(s, idmap) & (s != ONES)]  # (the twins of the pairs are stored)
    assert s.size > 3 * cs.n and np.isin(s & U64(0xFFFFFFFF), idmap & U64(0xFFFFFFFF)).all()
    assert idx.remove_ids(np.random.default_rng(4202).permutation(s)) == 0
    assert len(idx) == cs.n and idx.save_to_bytes() == blob
    idx.close()


@pytest.mark.parametrize("first_id", [pytest.param(2 ** 40 + 5, id="2p40"), pytest.param(2 ** 63 + 7, id="2p63"),
                                      pytest.param(None, id="up_to_2p64_minus_2")])
def test_append_writes_64_bit_ids_from_a_large_first_id(first_id):
    cs = Case(64, 7, 0, 1, True, OLD, ADD, 4300)
    first_id = 2 ** 64 - 1 - cs.n_add if first_id is None else first_id  # the last case ends on 2^64 - 2
    want = cs.one_shot()
    idx = cs.one_shot(cs.n_old)
    idx.add(cs.xd[cs.n_old:], cs.ad[cs.n_old:], first_id=first_id)
    idmap = np.concatenate([np.arange(cs.n_old, dtype=U64), U64(first_id) + np.arange(cs.n_add, dtype=U64)])
    assert int(idmap[-1]) == first_id + cs.n_add - 1
    _same_but_ids(want, idx, idmap, "large first_id")  # the ids that were written, as 64-bit values, not the cached bound
    assert idx.id_bound() == first_id + cs.n_add
    blob = idx.save_to_bytes()
    assert blob == _stream(cs.built, _clusters(cs.built, idmap))
    loaded = rq.IvfRabitqIndex.load_from_bytes(blob)
    assert loaded.id_bound() == first_id + cs.n_add  # the reduction
    loaded.close()
    # the largest new id goes: the bound is recomputed, here and on a handle loaded from the saved bytes
    assert idx.remove_ids(np.array([first_id + cs.n_add - 1, first_id - 1, first_id + cs.n_add], U64)) == 1
    assert idx.id_bound() == first_id + cs.n_add - 1
    K = np.arange(cs.n - 1)
    shrunk = _one_shot_rows(cs, K)
    _same_but_ids(shrunk, idx, idmap[K], "large first_id, the last id removed")
    loaded = rq.IvfRabitqIndex.load_from_bytes(idx.save_to_bytes())
    assert loaded.id_bound() == first_id + cs.n_add - 1
    want.close(); idx.close(); shrunk.close(); loaded.close()


def test_ids_that_would_pass_2p64_minus_1_are_refused():
    cs = Case(64, 7, 0, 1, True, OLD, ADD, 4350)
    idx = cs.one_shot(cs.n_old)
    before = _results(idx, cs.q, 10, cs.nl)
    arrays = {k: v.tobytes() for k, v in _arrays(idx).items()}
    # first_id + count = 2^64 + 1, 2^64 exactly (the last id would be the pad marker), and far past it
    for first_id in (2 ** 64 - cs.n_add + 1, 2 ** 64 - cs.n_add, 2 ** 64 - 1):
        with pytest.raises(rq.RabitqError) as e:
            idx.add(cs.xd[cs.n_old:], cs.ad[cs.n_old:], first_id=first_id)
        assert e.value.kind == "InvalidConfig" and "pass 2^64 - 1" in str(e.value), first_id
    after = _results(idx, cs.q, 10, cs.nl)
    assert len(idx) == cs.n_old and idx.id_bound() == cs.n_old
    assert {k: v.tobytes() for k, v in _arrays(idx).items()} == arrays
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    idx.close()


# ---- C. large removal sets ---------------------------------------------------------------------------------------------------
# rocprim's radix_sort_keys (device_radix_sort.hpp, radix_sort_impl) sorts up to 256 x 4 = 1 024 keys in one block, up to
# merge_sort_limit = 1 048 576 (device_radix_sort_config.hpp) by its merge sort, and more by onesweep: one size just below and one
# just above each switch.
SET_SIZES = [1, 2, 1024, 1025, 200_000, 1 << 20, (1 << 20) + 1, 3_000_000]


@pytest.fixture(scope="module")
def geo_sets():
    """the geometry-edge case, its reference set S, and the one-shot builds of the rows that stay without S and without S[:1]"""
    cs, S = _geo_case(64, 7, 0, 1, True, 4400)
    refs = {}
    for name, s in (("S", S), ("S1", S[:1])):
        K = _kept(cs.n, s)
        refs[name] = (s, K, _one_shot_rows(cs, K))
    yield cs, refs
    for _, _, h in refs.values():
        h.close()


def _big_set(S, n, m, seed):
    """m ids: S repeated to about half of m, ids in [n, 4n) (not stored), random 64-bit values (not stored either) and the pad
    marker, shuffled"""
    rng = np.random.default_rng(seed)
    part = np.tile(S, max(1, (m // 2) // S.size))
    rest = m - part.size - 1
    assert rest > 0
    r = np.frombuffer(rng.bytes(8 * (rest - rest // 2)), U64).copy()
    r[r < U64(4 * n)] += U64(4 * n)
    s = np.concatenate([part, rng.integers(n, 4 * n, rest // 2).astype(U64), r, np.array([ONES], U64)])
    assert s.size == m and np.array_equal(np.intersect1d(s, np.arange(n, dtype=U64)), np.sort(S))
    return rng.permutation(s)


@pytest.mark.parametrize("m,where", [(m, "host") for m in SET_SIZES] + [(m, "device") for m in SET_SIZES[-4:]])
def test_large_sets_with_repeats_and_unknown_ids_remove_exactly_the_reference_set(m, where, geo_sets):
    import torch
    cs, refs = geo_sets
    S, K, want = refs["S" if m > 2 else "S1"]
    if m <= 2:  # a set smaller than S: its first id, and one id that is not stored
        s = np.concatenate([S, np.array([cs.n + 5], U64)])[:m]
    else:
        s = _big_set(S, cs.n, m, 4400 + m % 1000)
    assert s.size == m
    idx = cs.one_shot()
    removed = idx.remove_ids(s if where == "host" else torch.from_numpy(s.view(np.int64)).cuda())
    assert removed == S.size and len(idx) == len(K)
    _same_but_ids(want, idx, K, f"set of {m}")
    idx.close()


# ---- D. sequences against a model --------------------------------------------------------------------------------------------
class _Model:
    """the live (id, row) pairs, in ascending id order: every append goes above the bound.  Every list is in ascending id order by
    contract, so the index after any step is the one-shot build over the live rows in this order, its ids j standing for ids[j]."""

    def __init__(self, cs):
        self.cs, self.ids, self.rows, self.next_row = cs, np.arange(cs.n_old, dtype=U64), np.arange(cs.n_old), cs.n_old

    def lists(self):
        return self.cs.assign[self.rows]

    def counts(self):
        return np.bincount(self.lists(), minlength=self.cs.nl)

    def ids_of(self, c):
        return self.ids[self.lists() == c]

    def bound(self):
        return int(self.ids.max()) + 1

    def remove(self, gone):
        keep = ~np.isin(self.ids, gone)
        self.ids, self.rows = self.ids[keep], self.rows[keep]
        return int((~keep).sum())

    def take(self, k):
        """the next k unused rows of the case"""
        r0, self.next_row = self.next_row, self.next_row + k
        assert self.next_row <= self.cs.n, "the case has too few spare rows"
        return r0, self.next_row

    def append(self, r0, r1, lists, first_id):
        assert first_id >= self.bound()
        self.cs.assign[r0:r1] = lists
        new = U64(first_id) + np.arange(r1 - r0, dtype=U64)
        self.ids, self.rows = np.concatenate([self.ids, new]), np.concatenate([self.rows, np.arange(r0, r1)])
        return new


@pytest.mark.parametrize("dim,bits,metric,faster", [
    pytest.param(64, 7, 0, True, id="d64_7bit_L2_const"),
    pytest.param(130, 3, 1, False, id="d130_3bit_IP_optimal_tail_granule"),
])
def test_removals_and_appends_in_sequence_follow_the_model(dim, bits, metric, faster):
    """Thirteen steps; their order is fixed, so that every kind of step runs in both cases and each finds the state it needs; the
    lists, ids and counts a step touches are drawn from the seed.  After step 7 the index is saved and loaded and the walk goes
    on with the loaded handle, for which the contract is on saved bytes and search results."""
    seed = 4500 + dim
    cs = Case(dim, bits, metric, 1, faster, OLD, ADD, seed, mult=2)  # 616 rows in 12 lists; the 466 further rows are spares
    rng = np.random.default_rng(seed + 7)
    m = _Model(cs)
    box = {"idx": cs.one_shot(cs.n_old), "loaded": False}
    appended = {}

    def check(step):
        idx = box["idx"]
        want = _one_shot_rows(cs, m.rows)
        assert len(idx) == len(m.ids) and idx.id_bound() == m.bound(), step
        ln = idx.debug_copy_index("list_n", np.empty(cs.nl, np.uint32))
        assert np.array_equal(ln, m.counts()), step
        if not box["loaded"]:
            _same_but_ids(want, idx, m.ids, f"step {step}")
        assert idx.save_to_bytes() == _writer_bytes(cs, m.rows, _row_ids(m), bits, metric, 1, seed), f"step {step}: saved bytes"
        _same_results(want, idx, cs.q, m.ids, nprobe=cs.nl, what=f"step {step}")
        want.close()

    def _row_ids(model):
        idmap = np.zeros(cs.n, U64)
        idmap[model.rows] = model.ids
        return idmap

    def remove(step, gone):
        gone = np.asarray(gone, U64)
        noise = np.array([m.bound() + 3, m.bound() + 2 ** 40, ONES], U64)  # ids that are not stored
        want = m.remove(gone)
        assert want == gone.size and len(m.ids) > 0
        assert box["idx"].remove_ids(rng.permutation(np.concatenate([gone, noise, gone[::3]]))) == want, step
        check(step)

    def append(step, lists, first_id, count=None):
        """lists: the list of every new row, or None for the nearest centroid of `count` rows"""
        r0, r1 = m.take(len(lists) if lists is not None else count)
        got = box["idx"].add(cs.xd[r0:r1], None if lists is None else np.asarray(lists, np.uint32), first_id=first_id,
                             rescale=cs.rescale, t_const=cs.t)
        if lists is not None:
            assert np.array_equal(got, lists), step
        appended[step] = m.append(r0, r1, got, first_id)
        check(step)

    def fill(step):
        """exactly as many rows as fill the partial tail block of a list"""
        n = m.counts()
        c = int(rng.choice(np.nonzero(n % 32 != 0)[0]))
        append(step, np.full(32 - n[c] % 32, c), m.bound())
        assert m.counts()[c] % 32 == 0

    check("start")
    remove(0, rng.choice(m.ids, len(m.ids) * 3 // 10, replace=False))                   # a random subset
    fill(1)                                                                             # fills a tail block step 0 left partial
    append(2, rng.integers(0, cs.nl, 80), m.bound())                                    # explicit lists, at the bound
    n = m.counts()
    c = int(rng.choice(np.nonzero((n > 32) & (n % 32 != 0))[0]))
    remove(3, m.ids_of(c)[-(n[c] % 32):])                                               # exactly the tail block of a list
    assert m.counts()[c] == n[c] - n[c] % 32
    live = appended[2][np.isin(appended[2], m.ids)]                                     # (step 3 may have taken some)
    remove(4, rng.choice(live, 40, replace=False))                                      # ids appended two steps earlier
    append(5, rng.integers(0, cs.nl, 50), m.bound() + 1000)                             # a gap above the bound
    # the nearest rotated centroid: the model takes the returned lists as given (the assignment itself is checked against
    # tests/kmeans_ref.py in tests/test_gpu_append.py)
    append(6, None, m.bound(), count=30)
    emptied = int(rng.choice(np.nonzero(m.counts() >= 33)[0]))
    remove(7, m.ids_of(emptied))                                                        # all of a list
    assert m.counts()[emptied] == 0

    blob = box["idx"].save_to_bytes()
    box["idx"].close()
    box["idx"], box["loaded"] = rq.IvfRabitqIndex.load_from_bytes(blob), True
    check("loaded")

    append(8, np.full(40, emptied), m.bound())                                          # refills the list step 7 emptied
    remove(9, rng.choice(m.ids, len(m.ids) // 4, replace=False))
    fill(10)
    append(11, None, m.bound(), count=60)                                               # nearest centroid, on the shrunk handle
    remove(12, np.concatenate([appended[10], appended[11][::2]]))                       # step 10's ids, two steps earlier
    box["idx"].close()


# ---- E. the old handle beside a mutation -------------------------------------------------------------------------------------
def test_old_handle_searches_and_fetches_beside_an_append_and_a_removal():
    cs = Case(64, 7, 0, 1, True, OLD, ADD, 4600, mult=2)
    old = cs.one_shot(cs.n_old)
    every = np.arange(cs.n_old, dtype=U64)
    emb0, found0 = old.fetch_embeddings(every)
    assert found0.all()
    base = old.batch_search_raw(cs.q, rq.SearchParams(10, cs.nl))
    gone = np.random.default_rng(4601).choice(cs.n_old, cs.n_old // 3, replace=False).astype(U64)
    mode, t = _rescale(cs.rescale, cs.t)
    bad = []

    def searcher():
        try:
            for _ in range(200):
                r = old.batch_search_raw(cs.q, rq.SearchParams(10, cs.nl))
                if not (np.array_equal(r[0], base[0]) and r[1].tobytes() == base[1].tobytes() and np.array_equal(r[2], base[2])):
                    bad.append("search")
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            bad.append(repr(e))

    def fetcher():
        try:
            for _ in range(40):
                o, f = old.fetch_embeddings(every)
                if not (f.all() and o.tobytes() == emb0.tobytes()):
                    bad.append("fetch")
        except Exception as e:  # noqa: BLE001
            bad.append(repr(e))

    threads = [threading.Thread(target=searcher), threading.Thread(target=fetcher)]
    grown, shrunk = [], []
    for th in threads:
        th.start()
    try:
        for _ in range(6):  # through the C entry: add() and remove_ids() would close the old handle
            h, out = C.c_void_p(), np.empty(cs.n_add, np.uint32)
            _check(lib().rbq_index_append(old._h, C.c_void_p(cs.xd[cs.n_old:].data_ptr()), C.c_void_p(cs.ad[cs.n_old:].data_ptr()),
                                          cs.n_add, cs.n_old, mode, t, 0, 1, None, out.ctypes.data, C.byref(h)))
            grown.append(rq.IvfRabitqIndex(h))
            h, removed = C.c_void_p(), C.c_uint64()
            _check(lib().rbq_index_remove_ids(old._h, gone.ctypes.data, gone.size, 1, None, C.byref(removed), C.byref(h)))
            shrunk.append(rq.IvfRabitqIndex(h))
            assert removed.value == gone.size and np.array_equal(out, cs.assign[cs.n_old:])
    finally:
        for th in threads:
            th.join()
    assert not bad, bad
    after = old.batch_search_raw(cs.q, rq.SearchParams(10, cs.nl))
    assert np.array_equal(after[0], base[0]) and after[1].tobytes() == base[1].tobytes()
    K = _kept(cs.n_old, gone)
    want_grown, want_shrunk = cs.one_shot(), _one_shot_rows(cs, K)
    for g, s in zip(grown, shrunk):
        _same_index(want_grown, g, "appended beside searches")
        _same_but_ids(want_shrunk, s, K, "shrunk beside searches")
    for i in grown + shrunk + [old, want_grown, want_shrunk]:
        i.close()
