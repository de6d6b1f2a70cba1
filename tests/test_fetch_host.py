"""fetch_embedding's CPU side: the numpy restatement (tests/fetch_ref.py) against the rotators of the CPU builder and the
crate's own sanity properties (src/tests.rs:1619-1735), and the Rust binding's new methods.  CPU only."""
import os
import re

import numpy as np
import pytest

import fetch_ref
import rabitq_rs_amd as rq
import rbq1_writer
from conftest import make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rot,dim", [(1, 64), (1, 128), (1, 100), (1, 200), (1, 960), (0, 64), (0, 96)],
                         ids=["fhtkac-64", "fhtkac-128", "fhtkac-100", "fhtkac-200", "fhtkac-960", "matrix-64", "matrix-96"])
def test_inverse_undoes_rotate(rot, dim):
    """inverse_rotate(rotate(x)) == x up to rounding (dim 100 and 200 take FHT-Kac's second case: trunc_dim < padded_dim)"""
    built = rq.builder.train(make_dataset(200, dim, 4, dim), 4, 1, 0, rot, 5 + dim, True, kmeans_iters=2)
    x = np.random.default_rng(dim).standard_normal((6, dim)).astype(np.float32)
    r = np.stack([built.rotate(v) for v in x])
    back = fetch_ref.inverse_rotate(dim, built.padded_dim, rot, built.rotator_blob(), r)
    assert back.shape == x.shape and back.dtype == np.float32
    assert np.abs(back - x).max() <= 1e-4 * np.abs(x).max(), np.abs(back - x).max()
    built.close()


def _rel_errors(data, out):
    return np.linalg.norm(out - data, axis=1) / np.maximum(np.linalg.norm(data, axis=1), np.finfo(np.float32).eps)


@pytest.mark.parametrize("rot,dim,n,nlist,seed", [(0, 64, 100, 4, 12345), (1, 128, 50, 8, 54321)], ids=["matrix-64", "fhtkac-128"])
def test_crate_sanity_properties(rot, dim, n, nlist, seed):
    """test_fetch_embedding_reconstruction / _fht_rotator: 7 bits, optimal rescale; every id comes back with a relative
    error below 2.0, and an id past the end is not found"""
    data = np.random.default_rng(seed).random((n, dim), dtype=np.float32) * 2 - 1
    built = rq.builder.train(data, nlist, 7, 0, rot, seed, False, kmeans_iters=10)
    stream = rbq1_writer.from_built(built)
    out, found = fetch_ref.fetch(stream, np.arange(n + 11))
    assert found[:n].all() and not found[n:].any()
    assert out.shape == (n + 11, dim)
    assert (_rel_errors(data, out[:n]) < 2.0).all()
    assert not out[n:].any()
    built.close()


def test_first_occurrence_wins_and_sparse_ids():
    """a stream whose ids repeat across clusters: the first (cluster, position) occurrence is the one decoded"""
    built = rq.builder.train(make_dataset(300, 64, 4, 3), 4, 3, 0, 1, 9, True, kmeans_iters=3)
    stream = built.save_rbq1()
    ref = fetch_ref.Rbq1(stream)
    ids = fetch_ref.all_ids(ref)
    c0, c1 = ref.clusters[0], ref.clusters[1]
    dup = int(c1["ids"][0])
    c0["ids"][-1] = dup  # the same id, earlier in (cluster, position) order
    out, found = fetch_ref.fetch(ref, [dup, 1 << 40])
    assert found.tolist() == [True, False]
    want = fetch_ref.inverse_rotate(ref.dim, ref.padded_dim, ref.rotator, ref.rot,
                                    fetch_ref.rotated(ref, 0, len(c0["ids"]) - 1)[None])[0]
    assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
    assert len(ids) == len(built)
    built.close()


def test_rust_binding_has_the_fetch_methods():
    rs = open(os.path.join(ROOT, "integration", "gpu_ivf.rs")).read()
    for needle in ("pub fn fetch_embedding(&self, vector_id: usize) -> Option<Vec<f32>>",
                   "pub fn fetch_embeddings(&self, ids: &[usize]) -> Result<Vec<Option<Vec<f32>>>, RabitqError>",
                   "fn rbq_index_fetch_embeddings(", "fn rbq_index_fetch_embeddings_device("):
        assert needle in rs, needle
    hdr = open(os.path.join(ROOT, "include", "rbq.h")).read()
    assert re.search(r"int rbq_index_fetch_embeddings\(const rbq_index\* idx, const uint64_t\* ids, uint64_t n, float\* out, "
                     r"uint8_t\* found\);", hdr)
    assert "rbq_index_fetch_embeddings_device(" in hdr
