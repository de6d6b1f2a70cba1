"""The catalogue of tests/call_sequence_cases.py on the CPU oracle alone: the checks that keep the GPU tests of
tests/test_gpu_call_sequences.py from being hollow.  A kind whose reference were empty, or equal to another
kind's, could be served from the other call's leftovers without a test noticing."""
import itertools

import numpy as np
import pytest

import call_sequence_cases as cs
import oracle
from call_sequence_cases import BY_NAME, KINDS, ROUTES, bits, case, kinds_of, reference

RANGE = ("range", "range_exact")


def _probed_vectors(kind):
    """vectors a query of this kind can reach at most: those of its nprobe largest lists"""
    sizes = sorted((int(s) for s in case(kind.index).built.list_sizes()), reverse=True)
    return sum(sizes[:min(kind.nprobe, len(sizes))])


@pytest.mark.parametrize("name", [k.name for k in KINDS])
def test_reference_is_not_hollow(name):
    """the rule of the GPU test accepts the reference itself; the reference has a full row and a non-empty row (a top_k beyond the
    probed vectors: the fullest row holds more than half of them and is padded after; range: see test_range_kinds)"""
    kind = BY_NAME[name]
    ref = reference(name)
    cs.check(kind, cs.as_result(ref))
    assert ref.ids.shape == (kind.rows[1], ref.top_k) and ref.counts.shape == (kind.rows[1],)
    assert (ref.counts > 0).any(), "no non-empty row"
    if kind.mode in RANGE:
        return
    if kind.top_k <= _probed_vectors(kind) and kind.filt is None:
        assert (ref.counts == kind.top_k).any(), "no full row"
    else:
        assert ref.counts.max() > min(kind.top_k, _probed_vectors(kind)) // 8
    if (ref.counts < kind.top_k).any():  # a padded row is padded with the two patterns the library writes
        q = int(np.nonzero(ref.counts < kind.top_k)[0][0])
        assert ref.ids[q, -1] == cs.PAD_ID and bits(ref.scores)[q, -1] == cs.NAN_BITS


def test_every_why_names_its_reason():
    for k in KINDS:
        assert k.why.strip(), k.name
        for o in k.opts:
            assert len(o) == 3 and o[1] != o[2], (k.name, o)
    assert {k.index for k in KINDS} == {"A", "B", "C", "P"}
    assert all(BY_NAME[n].entry == "device" for n in ROUTES)


@pytest.mark.parametrize("name", [k.name for k in KINDS if k.filt])
def test_filtered_kinds_drop_something(name):
    kind = BY_NAME[name]
    keep, fw, nbits = cs.filter_of(kind)
    ref = reference(name)
    c = case(kind.index)
    wq = cs.queries(kind)[1]
    valid = ref.ids != cs.PAD_ID
    assert all(int(i) in keep for i in ref.ids[valid]), "a returned id is not allowed"
    if kind.mode in RANGE:
        import range_ref
        free = range_ref.range_batch(c.built, wq, cs.radii(name)[0], kind.nprobe)
        assert sum(len(r[0]) for r in free) > int(ref.counts.sum()) > 0
    else:
        rc, ids, _, cnt, _ = oracle.search_batch(c.built, wq, kind.top_k, kind.nprobe)
        assert rc == 0
        dropped = [int(i) for i in ids[ids != cs.PAD_ID] if int(i) not in keep]
        assert len(dropped) > len(wq), "the filter drops fewer than one result per query"
    if kind.filt == "short":
        assert nbits < len(c.data) and any(int(i) >= nbits for i in ids[ids != cs.PAD_ID]), "no result beyond the filter's length to drop"


@pytest.mark.parametrize("name", [k.name for k in KINDS if k.mode in RANGE])
def test_range_kinds(name):
    """a query without a match, one with more than a half-wave's worth; a capacity below the totals cuts rows, one above cuts none"""
    kind = BY_NAME[name]
    ref = reference(name)
    assert (ref.counts == 0).any(), "no query without a match"
    if kind.mode == "range":
        assert (ref.counts > 32).any(), "no query with more than 32 matches"
    else:  # the exact radius at the first row's 21st exact score: the rows reject candidates
        cand = sum(int(r[2][0]) for r in ref.probed)
        assert (ref.counts >= 16).any() and cand > int(ref.counts.sum())
    if kind.top_k:
        assert (ref.counts > kind.top_k).any() and ((ref.counts > 0) & (ref.counts < kind.top_k)).any(), "the capacity cuts no row, or every row"
    else:
        assert ref.counts.max() < ref.top_k


def test_degenerate_kind():
    """what tests/test_gpu_round4.py::test_degenerate_queries expects is the oracle's answer; here: the rows are what they are
    meant to be, the oracle answers them, the copy of a stored vector finds it (and its duplicate) first and the ordinary row is full"""
    kind = BY_NAME["a_degenerate"]
    q = cs.queries(kind)[1]
    assert not q[0].any() and np.isnan(q[1]).sum() == 1 and np.isnan(q[2]).all() and np.isinf(q[3]).sum() == 1 and np.isinf(q[4]).all()
    assert np.array_equal(q[5], case("A").data[100]) and np.signbit(q[6]).all() and np.isfinite(q[7]).all()
    ref = reference(kind.name)
    rc, ids, sc, cnt, diag = oracle.search_batch(case("A").built, q, kind.top_k, kind.nprobe, want_diag=True)
    assert rc == 0 and np.array_equal(ids, ref.ids) and np.array_equal(cnt, ref.counts) and np.array_equal(diag, ref.diag)
    assert sorted(ref.ids[5, :2].tolist()) == [100, 5999] and ref.counts[5] == 10 and ref.counts[7] == 10 and ref.counts[0] == 10
    assert np.array_equal(ref.ids[0], ref.ids[6]), "+0 and -0 queries answer alike"


@pytest.mark.parametrize("name", ["a_exact_heap", "a_tie_log0"])
def test_tie_kinds_have_ties(name):
    ref = reference(name)
    s = bits(ref.scores)
    tied = [(s[q, 1:int(c)] == s[q, :int(c) - 1]).any() for q, c in enumerate(ref.counts)]
    assert sum(tied) >= 2, "fewer than two queries with two equal distances in their top-k"
    assert sorted(ref.ids[0, :2].tolist()) == [100, 5999] and sorted(ref.ids[1, :2].tolist()) == [101, 5998]


def _fingerprint(ref):
    return (ref.ids.shape, ref.ids.tobytes(), bits(ref.scores).tobytes(), ref.counts.tobytes(), None if ref.diag is None else ref.diag.tobytes())


@pytest.mark.parametrize("index", ["A", "B", "C", "P"])
def test_no_two_references_of_an_index_are_equal(index):
    """in shape, rows or padding: the result of one kind cannot pass for another's; beyond that, two kinds of one shape differ in
    more than a quarter of their rows"""
    ks = kinds_of(index)
    fp = {k.name: _fingerprint(reference(k.name)) for k in ks}
    for a, b in itertools.combinations(ks, 2):
        assert fp[a.name] != fp[b.name], f"{a.name} and {b.name} have the same reference"
        ra, rb = reference(a.name), reference(b.name)
        if ra.ids.shape == rb.ids.shape and index != "P":
            differ = ((ra.ids != rb.ids).any(axis=1) | (ra.counts != rb.counts)).mean()
            assert differ > 0.25, f"{a.name} and {b.name} differ in {differ:.0%} of their rows only"


def test_the_routes_table_covers_the_design_rows():
    """one kind at least per row of the DESIGN section 31 table that indexes of these sizes reach, by the table's own columns"""
    r = ROUTES
    assert any(v.get("rank", 0) is None for v in r.values())                              # latency front
    assert {v.get("parts") for v in r.values()} >= {1, 2, 4}                              # split-K parts, by rule and forced
    assert {v.get("rank") for v in r.values()} >= {None, "f32", "bf16x3", "f16"}         # every ranking route
    assert {v["scan"] for v in r.values()} == {64, 256}                                   # k_scanw, k_scan / k_range
    assert r["a_nq513"]["prep"] == (513 + 3) // 4 and r["a_nq200_lat0"]["prep"] == 50      # k_prep_wave: four queries per workgroup
    assert any(k.nprobe > 8192 for k in KINDS) and any(k.top_k > 16384 for k in KINDS)    # big_nprobe, the heap in global memory
