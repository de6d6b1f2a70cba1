"""The cases of the scan-instantiation sweep (tests/scan_instantiation_cases.py) exercise what the GPU test believes they do:
conditions on the CPU oracle alone, for every (dim, bits, metric, top_k) of tests/test_gpu_scan_instantiations.py, so that the
GPU test cannot pass on a degenerate case.  No GPU."""
import numpy as np
import pytest

import oracle
import scan_instantiation_cases as sic


def _distinct(row):
    return len(np.unique(row.view(np.uint32))) == len(row)


@pytest.mark.parametrize("bits", sic.BITS)
@pytest.mark.parametrize("dim", sic.DIMS)
def test_cases_exercise_ties_skips_and_refinement(dim, bits):
    for metric in sic.METRICS:
        data, built, q = sic.case(dim, bits, metric)
        what = f"dim {dim} bits {bits} metric {metric}"
        assert data.shape == (sic.N, dim) and q.shape == (sic.NQ, dim)
        assert built.padded_dim == dim, what  # the compile-time instantiation of this dimension serves, not the runtime one
        assert built.n_lists == sic.NLIST and int(built.header.ex_bits) == bits - 1
        for top_k in sic.TOP_KS:
            rc, ids, sc, cnt, diag = oracle.search_batch(built, q, top_k, sic.NPROBE, want_diag=True)
            assert rc == 0
            w = f"{what} top_k {top_k}"
            assert (cnt == top_k).all(), f"{w}: rows not full: {cnt}"
            tied = sum(not _distinct(sc[i]) for i in range(sic.NQ_DUP))
            assert tied == sic.NQ_DUP, f"{w}: {tied} of {sic.NQ_DUP} duplicate queries have two equal scores"
            free = sum(_distinct(sc[i]) for i in range(sic.NQ_DUP, sic.NQ))
            assert free >= 21, f"{w}: {free} of {sic.NQ_FAR} far queries are tie-free"
            assert (diag[:, 1] >= 1).all(), f"{w}: a query skips nothing by the lower bound: {diag[:, 1]}"
            if bits > 1:
                assert (diag[:, 2] > top_k).all(), f"{w}: extended evaluations {diag[:, 2]}"
        # the filtered calls: every third id, which admits components 0 and 3 whole and nothing of the others (the components are
        # dealt round-robin): the duplicate queries' rows are full, some far queries' rows are short or empty, only allowed ids come back
        words, nbits = sic.filter_words()
        for top_k in sic.FILTERED_TOP_KS:
            rc, ids, sc, cnt, _ = oracle.search_batch(built, q, top_k, sic.NPROBE, words, nbits)
            assert rc == 0 and (cnt[:sic.NQ_DUP] == top_k).all(), f"{what} filtered top_k {top_k}: {cnt}"
            assert all((ids[i, :int(cnt[i])] % 3 == 0).all() for i in range(sic.NQ))
