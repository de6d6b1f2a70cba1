"""All outputs of the three query-preparation kernels, held together on one input.

k_prep (a workgroup per query; the only one that serves the matrix rotator), k_prep_wave (a wave per query) and k_lat_front (the
latency front, and the workgroup-per-query preparation of medium batches) share their steps as device functions
(query_kernels.hpp) and differ in structure.  For the same five queries the preparation runs through
  wg_prep = 1          k_prep
  latency_path = 0     k_prep_wave: five queries leave a partial last workgroup, the wave with q >= nq leaves
  defaults             k_lat_front as a preparation only (5 > kLatMaxQueries)
  three queries alone  k_lat_front with its scorers ([0, 1, 2] and [2, 3, 4])
and the route is asserted from stage_resources().  Compared bit for bit: rot and lut (padding tables zero); consts, all 12 words
between k_prep_wave and k_lat_front and all but q1norm / exlo / exhi between k_prep and those two; the split-bf16 image rot_hl; with
rank_f16 = 1 the f16 image rot_f16 and rank_resid.  k_prep adds the positive and the negative elements serially on one thread, so its
q1norm, exlo and exhi are held to a host restatement of that order over the device's own rot row.
k_prep rotates with the LDS butterflies and flip passes of their own, the other two with the in-register transform that fuses the
flips into its loads: a NaN element leaves the two with either sign.  So between k_prep and the other two the elements of a query
that are NaN in both compare as NaN (in rot, in the images at the same element, in consts and rank_resid); everything else, and
everything between k_prep_wave and k_lat_front, is compared bit for bit.
Queries: two ordinary ones, one all-zero (delta == 0: emin = 0), one with a NaN element, one scaled by 1e30.
Shapes (2000 vectors, 16 lists, 7 bits): dim 64 (the transform covers the vector: one element per lane), 192 (transform of 128 and
the Kac steps), 100 (padded to 128), 40 (padded to 64, transform of 32: the generic LDS butterflies), and the matrix rotator, which
only k_prep serves, against the oracle's stage functions: dim 64, and dim 80, whose code layout is padded to 128 so that padding
codebooks are written (an FHT-Kac index is padded to a multiple of 64 and has none)."""
import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
from conftest import build_index, make_dataset

pytestmark = pytest.mark.gpu

N, NLIST, BITS, TOP_K, NPROBE, NQ = 2000, 16, 7, 10, 4, 5
Q1NORM_EXLO_EXHI = [7, 8, 9]  # words of QueryConsts: delta sum_vl k1x kbx scale qnorm | qnorm2 exlo exhi q1norm amin amax
OTHER_WORDS = [w for w in range(12) if w not in Q1NORM_EXLO_EXHI]
OPTS = {"k_prep": {"wg_prep": 1, "latency_path": 1}, "k_prep_wave": {"wg_prep": 0, "latency_path": 0},
        "k_lat_front": {"wg_prep": 0, "latency_path": 1}}


def _queries(dim, metric, seed):
    q = make_dataset(NQ, dim, 4, seed, normalize=(metric == 1))
    q[2] = 0.0
    q[3, 5] = np.nan
    q[4] *= np.float32(1e30)
    return q


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b, what):
    bad = np.argwhere(_bits(a) != _bits(b))
    assert bad.size == 0, f"{what}: {len(bad)} element(s) differ, first at {bad[0].tolist()}"


def _same_but_nan(a, b, nan, what):
    """bit for bit, except where `nan` (same shape) marks an element that is NaN on both sides"""
    bad = np.argwhere((_bits(a) != _bits(b)) & ~nan)
    assert bad.size == 0, f"{what}: {len(bad)} element(s) differ, first at {bad[0].tolist()}"


def _both_nan(a, b):
    return np.isnan(a) & np.isnan(b)


def _hl_mask(nan, D):
    """`nan` [nq][D] per element -> per u16 of the split-bf16 image [nq][2 D]: slab s holds hi of elements 32 s .. 32 s + 31, then lo"""
    p = np.arange(2 * D)
    return nan[:, (p // 64) * 32 + p % 32]


class _Runner:
    def __init__(self, built, q):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.idx = rq.IvfRabitqIndex.from_built(built)
        self.q, self.dim = q, q.shape[1]
        self.D = built.padded_dim
        self.Dc = (self.D + 63) // 64 * 64
        self.st = torch.cuda.Stream(self.dev)

    def run(self, opts, rows, f16):
        """one call with the queries `rows` under `opts`; returns (stage resources, the preparation's outputs)"""
        torch, idx, s, D = self.torch, self.idx, self.st.cuda_stream, self.D
        for k, v in dict(opts, rank_f16=1 if f16 else 0).items():
            idx.set_option(k, v)
        nq = len(rows)
        qd = torch.from_numpy(np.ascontiguousarray(self.q[rows])).to(self.dev)
        out = (torch.zeros(nq, TOP_K, dtype=torch.int64, device=self.dev), torch.zeros(nq, TOP_K, dtype=torch.float32, device=self.dev),
               torch.zeros(nq, dtype=torch.int32, device=self.dev))
        torch.cuda.synchronize(self.dev)
        idx.search_batch_device(qd.data_ptr(), nq, self.dim, TOP_K, NPROBE, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream=s)
        torch.cuda.synchronize(self.dev)
        res = idx.stage_resources(nq, TOP_K, NPROBE)
        taps = {"rot": idx.debug_copy_workspace(s, "rot", np.empty((nq, D), np.float32)),
                "lut": idx.debug_copy_workspace(s, "lut", np.empty((nq, self.Dc * 4), np.uint8)),
                "consts": idx.debug_copy_workspace(s, "consts", np.empty((nq, 12), np.float32))}
        if res["rank"]["operands"] == "f16":
            taps["rot_f16"] = idx.debug_copy_workspace(s, "rot_f16", np.empty((nq, D), np.uint16))
            taps["rank_resid"] = idx.debug_copy_workspace(s, "rank_resid", np.empty(nq, np.float32))
        elif res["rank"]["operands"] == "bf16x3":
            taps["rot_hl"] = idx.debug_copy_workspace(s, "rot_hl", np.empty((nq, 2 * D), np.uint16))
        return res, taps

    def close(self):
        self.idx.release_stream(self.st.cuda_stream)
        self.idx.close()


def _padding_is_zero(lut, D, Dc, what):
    # device LUT order: position p holds codebook p ^ 1; D / 4 is even, so the swap never mixes real and padding tables
    assert not lut.reshape(-1, Dc // 4, 16)[:, D // 4:].any(), f"{what}: a padding table is not zero"


def _kprep_own_words(row, ex_bits):
    """q1norm, exlo, exhi in k_prep's order: serial float32 sums of max(x, 0) and min(x, 0), then ex_dot_range's expression"""
    f = np.float32
    sp, sn = f(0.0), f(0.0)
    with np.errstate(all="ignore"):
        for v in row:
            sp = f(sp + np.fmax(v, f(0.0)))
            sn = f(sn + np.fmin(v, f(0.0)))
        cmax = f((1 << ex_bits) - 1)
        slack = f(f(cmax * f(sp - sn)) * f(1e-3))
        exlo, exhi = f(f(cmax * sn) - slack), f(f(cmax * sp) + slack)
        q1norm = f(f(sp - sn) * f(1.001))
    return np.array([exlo, exhi, q1norm], f)  # words 7, 8, 9


def _check_kprep_own_words(taps, ex_bits, what):
    for i in range(len(taps["rot"])):
        want, got = _kprep_own_words(taps["rot"][i], ex_bits), taps["consts"][i, Q1NORM_EXLO_EXHI]
        print(f"{what} query {i}: exlo exhi q1norm {got} host {want}")
        _same(got, want, f"{what} query {i}: exlo / exhi / q1norm against the serial restatement")


@pytest.mark.parametrize("dim,metric", [(64, 0), (192, 1), (100, 0), (40, 0)], ids=["d64_pow2_L2", "d192_kac128_IP", "d100_pad128_L2", "d40_lds_fht_L2"])
def test_three_kernels_agree(dim, metric):
    data, built = build_index(n=N, dim=dim, nlist=NLIST, total_bits=BITS, metric=metric, rotator=1, normalize=(metric == 1), seed=9100 + dim)
    r = _Runner(built, _queries(dim, metric, 9200 + dim))
    D, Dc, ex = r.D, r.Dc, built.hdr.ex_bits
    assert D % 64 == 0  # (FHT-Kac pads to 64: both GEMM images exist at every one of these shapes)
    allq = list(range(NQ))
    for f16 in (False, True):
        got = {k: r.run(OPTS[k], allq, f16) for k in OPTS}
        # ---- routes
        res = {k: v[0] for k, v in got.items()}
        for k in OPTS:
            assert res[k]["rank"]["operands"] == ("f16" if f16 else "bf16x3"), (k, res[k]["rank"])
            assert res[k]["prep"]["threads"] == 256
        assert res["k_prep"]["prep"]["workgroups"] == NQ and res["k_lat_front"]["prep"]["workgroups"] == NQ
        assert res["k_prep_wave"]["prep"]["workgroups"] == (NQ + 3) // 4
        assert res["k_prep"]["prep"]["lds_bytes"] != res["k_lat_front"]["prep"]["lds_bytes"]  # (the front holds the flip bits too)
        t = {k: v[1] for k, v in got.items()}
        image = ["rot_f16", "rank_resid"] if f16 else ["rot_hl"]
        # ---- k_prep_wave and k_lat_front: everything
        for name in ["rot", "lut", "consts"] + image:
            _same(t["k_prep_wave"][name], t["k_lat_front"][name], f"dim {dim} f16={f16} {name}: k_prep_wave vs k_lat_front")
        # ---- k_prep and those two: everything but its three words
        a, b = t["k_prep"], t["k_prep_wave"]
        nan = _both_nan(a["rot"], b["rot"])
        assert not nan[[0, 1, 2, 4]].any() and nan[3].any()
        what = f"dim {dim} f16={f16} %s: k_prep vs k_prep_wave"
        _same_but_nan(a["rot"], b["rot"], nan, what % "rot")
        _same(a["lut"], b["lut"], what % "lut")
        if f16:
            _same_but_nan(a["rot_f16"], b["rot_f16"], nan, what % "rot_f16")
            _same_but_nan(a["rank_resid"], b["rank_resid"], _both_nan(a["rank_resid"], b["rank_resid"]), what % "rank_resid")
        else:
            _same_but_nan(a["rot_hl"], b["rot_hl"], _hl_mask(nan, D), what % "rot_hl")
        ca, cb = a["consts"][:, OTHER_WORDS], b["consts"][:, OTHER_WORDS]
        _same_but_nan(ca, cb, _both_nan(ca, cb), what % "consts")
        _check_kprep_own_words(t["k_prep"], ex, f"dim {dim} f16={f16} k_prep")
        for k in OPTS:
            _padding_is_zero(t[k]["lut"], D, Dc, k)
        assert t["k_prep"]["consts"][2, 0] == 0.0 and not t["k_prep"]["lut"][2].any()  # the all-zero query: delta == 0, emin = 0
    # ---- k_lat_front with its scorers (no GEMM, no image): small calls against the rows of the five-query call
    whole = t["k_prep_wave"]
    for rows in ([0, 1, 2], [2, 3, 4]):
        res3, t3 = r.run(OPTS["k_lat_front"], rows, False)
        assert res3["rank"]["workgroups"] == 0 and res3["prep"]["lds_bytes"] == res["k_lat_front"]["prep"]["lds_bytes"]
        G = (NLIST + 31) // 32
        assert res3["prep"]["workgroups"] == (G + 1 + 7) // 8 * 8 * len(rows)
        for name in ("rot", "lut", "consts"):
            _same(t3[name], whole[name][rows], f"dim {dim} {name}: k_lat_front with scorers, queries {rows}, vs k_prep_wave")
        _padding_is_zero(t3["lut"], D, Dc, "k_lat_front with scorers")
    r.close()


def _same_or_nan(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))
    assert ok.all(), f"{what}: {a[~ok][:4]} vs {b[~ok][:4]}"


@pytest.mark.parametrize("dim", [64, 80], ids=["d64", "d80_padded_codebooks"])
def test_matrix_rotator_k_prep_matches_oracle_stages(dim):
    """The matrix rotator is served by k_prep alone: its outputs against the oracle's stage functions (as test_stage_level_parity
    does), its own three words against the serial restatement."""
    data, built = build_index(n=N, dim=dim, nlist=NLIST, total_bits=BITS, metric=0, rotator=0, seed=9300 + dim)
    q = _queries(dim, 0, 9400 + dim)
    r = _Runner(built, q)
    D, Dc, ex = r.D, r.Dc, built.hdr.ex_bits
    assert D == dim
    for opts in ({"wg_prep": 0, "latency_path": 1}, {"wg_prep": 0, "latency_path": 0}):  # k_prep whatever the options say
        res, t = r.run(opts, list(range(NQ)), False)
        assert res["prep"]["workgroups"] == NQ and res["prep"]["threads"] == 256
        for i in range(NQ):
            rot = oracle.rotate(built, q[i])
            _same_or_nan(t["rot"][i], rot, f"query {i}: rotated vector")
            lut, delta, sum_vl = oracle.query_lut(rot)
            dev_lut = t["lut"][i].reshape(Dc // 4, 16)
            ref_lut = lut.reshape(D // 4, 16)
            assert np.array_equal(dev_lut[np.arange(D // 4) ^ 1], ref_lut), f"query {i}: LUT bytes differ"
            qc = oracle.query_precompute(rot, ex)
            want = np.array([delta, sum_vl, qc.k1x_sum_q, qc.kbx_sum_q, qc.binary_scale, qc.query_norm], np.float32)
            _same_or_nan(t["consts"][i, :6], want, f"query {i}: consts")
            assert t["consts"][i, 10] == ref_lut.min(axis=1).astype(np.float64).sum() and t["consts"][i, 11] == ref_lut.max(axis=1).astype(np.float64).sum()
        _padding_is_zero(t["lut"], D, Dc, "k_prep")
        assert (Dc > D) == (dim == 80)
        _check_kprep_own_words(t, ex, f"matrix dim {dim} k_prep")
    r.close()
