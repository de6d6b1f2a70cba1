"""bench.py --dump-outputs: the last timed step's results, written as .npy files, are identical from run to run with the same
arguments (seeded inputs, deterministic harness k-means), and --steps is the number of timed steps.  One of the two runs is a
--full run (counter pass, roofline and per-stage pass behind the timed region), the other a plain one: the supplementary legs
change neither the timed steps nor what is dumped, and a plain run reports none of them."""
import os

import numpy as np
import pytest

from test_gpu_round3 import _run_bench

ARGS = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--no-extras", "--no-cpu", "--no-latency", "--nbatches", "3",
        "--n", "200000", "--nlist", "1024", "--nprobe", "32"]


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_exactly(tmp_path):
    runs = []
    for r, mode in enumerate((["--full"], [])):
        d = tmp_path / f"run{r}"
        res = _run_bench(ARGS + mode + ["--dump-outputs", str(d)], {})
        assert res["steps"] == 7 and res["timed_regions"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
        assert res["full"] == bool(mode) and res["recall_at_10"] > 0.9
        if mode:
            assert res["pruned"]["launches"] == 7 and res["roofline"]["ids_identical_to_product_configuration"]
        else:
            for k in ("pruned", "roofline", "regime", "stage_ms", "encoder", "host_call", "pcie_inclusive", "latency", "self_check",
                      "datasets", "sensitivity"):
                assert res[k] is None, k
            assert "cpu_baseline" not in res
        runs.append({n: np.load(d / f"{n}.npy") for n in ("ids", "scores", "counts", "queries", "rows")})
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    a, b = runs
    assert a["ids"].dtype == np.float64 and a["scores"].dtype == np.float32 and a["queries"].dtype == np.float32
    assert a["ids"].shape == a["scores"].shape == (1024, 10) and a["counts"].shape == (1024,) and a["queries"].shape == (1024, 960)
    assert (a["counts"] == 10).all()
    for n in a:
        assert np.array_equal(a[n], b[n], equal_nan=(n == "scores")), n
