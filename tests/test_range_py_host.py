"""rabitq_rs_amd/_range.py: what the range searches of the three index modules share on the Python side.  No GPU."""
import numpy as np
import pytest

from rabitq_rs_amd import _range
from rabitq_rs_amd.bruteforce import _filter_words as bf_filter_words
from rabitq_rs_amd.index import IvfRabitqIndex


def _words_by_hand(ids):
    """The bitset rule spelt out bit by bit: nbits = largest id + 1, ceil(nbits / 32) words and never none."""
    ids = set(int(i) for i in ids)
    nbits = max(ids) + 1 if ids else 0
    words = [0] * max((nbits + 31) // 32, 1)
    for i in ids:
        words[i >> 5] |= 1 << (i & 31)
    return np.array(words, np.uint32), nbits


@pytest.mark.parametrize("ids", [[], [0], [31, 32], [70, 3, 3, 64, 0, 70, 31]], ids=["empty", "zero", "word_edge", "unsorted_dups"])
def test_filter_words(ids):
    want, want_bits = _words_by_hand(ids)
    for fn in (_range.filter_words, IvfRabitqIndex._filter_words, bf_filter_words):
        words, nbits = fn(ids)
        assert nbits == want_bits and words.dtype == np.uint32 and np.array_equal(words, want)
    assert np.array_equal(_range.filter_words(np.asarray(ids, np.int64))[0], want)


def test_f32_bits():
    assert _range.f32_bits(1.0) == 0x3F800000 and _range.f32_bits(np.inf) == 0x7F800000
    assert _range.f32_bits(-0.0) == -0x80000000 and _range.f32_bits(0.1) == int(np.float32(0.1).view(np.int32))


class _Rows:
    """A fake range entry: query q has totals[q] matches, ids 100 q + rank; records the capacities it was called with."""

    def __init__(self, totals):
        self.totals, self.caps = np.asarray(totals, np.uint32), []

    def __call__(self, cap):
        self.caps.append(cap)
        ids = np.full((len(self.totals), cap), np.uint64(2**64 - 1))
        sc = np.full((len(self.totals), cap), np.nan, np.float32)
        for q, t in enumerate(self.totals):
            n = min(int(t), cap)
            ids[q, :n] = 100 * q + np.arange(n)
            sc[q, :n] = np.arange(n, 0, -1)
        return ids, sc, self.totals.copy(), "extra"


def test_complete_rows_repeats_once_at_the_largest_total():
    rows = _Rows([3, 2000, 1025, 0])
    got = _range.complete_rows(rows, None)
    assert rows.caps == [1024, 2000] and got[0].shape == (4, 2000) and got[3] == "extra"
    assert np.array_equal(got[2], rows.totals)


@pytest.mark.parametrize("totals", [[3, 1024, 0], [], [0]])
def test_complete_rows_without_a_repeat(totals):
    rows = _Rows(totals)
    _range.complete_rows(rows, None)
    assert rows.caps == [1024]


def test_complete_rows_with_max_results_calls_once():
    rows = _Rows([3, 2000])
    got = _range.complete_rows(rows, 5)
    assert rows.caps == [5] and got[0].shape == (2, 5)


@pytest.mark.parametrize("sort", [False, True])
def test_csr(sort):
    ids, sc, cnt, _ = _Rows([3, 0, 7, 4])(4)  # (the third row holds 4 of its 7)
    for fn in (_range.csr, IvfRabitqIndex._range_csr):
        lims, out_ids, out_sc = fn(ids, sc, cnt, sort)
        assert lims.dtype == np.int64 and lims.tolist() == [0, 3, 3, 7, 11]
        for q, n in enumerate([3, 0, 4, 4]):
            want = 100 * q + np.arange(n)
            want_sc = np.arange(n, 0, -1).astype(np.float32)
            if sort:  # ascending by score: the scan order reversed
                want, want_sc = want[::-1], want_sc[::-1]
            assert np.array_equal(out_ids[lims[q]:lims[q + 1]], want.astype(np.uint64))
            assert np.array_equal(out_sc[lims[q]:lims[q + 1]], want_sc)


def test_csr_sort_is_stable_on_equal_scores():
    ids = np.array([[5, 9, 7, 1]], np.uint64)
    sc = np.array([[2.0, 1.0, 2.0, 1.0]], np.float32)
    _, out_ids, out_sc = _range.csr(ids, sc, np.array([4], np.uint32), True)
    assert out_ids.tolist() == [9, 1, 5, 7] and out_sc.tolist() == [1.0, 1.0, 2.0, 2.0]
