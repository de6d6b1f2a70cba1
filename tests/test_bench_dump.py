"""bench.py --dump-outputs: the last timed step's results, written as .npy files, are identical from run to run with the same
arguments (seeded inputs, deterministic harness k-means), and --steps is the number of timed steps."""
import os

import numpy as np
import pytest

from test_gpu_round3 import _run_bench

ARGS = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--no-extras", "--no-cpu", "--no-latency", "--nbatches", "3",
        "--n", "200000", "--nlist", "1024", "--nprobe", "32"]


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_exactly(tmp_path):
    runs = []
    for r in range(2):
        d = tmp_path / f"run{r}"
        res = _run_bench(ARGS + ["--dump-outputs", str(d)], {})
        assert res["steps"] == 7 and res["timed_regions"] == 1 and res["pruned"]["launches"] == 7 and res["ms_per_step"] > 0
        runs.append({n: np.load(d / f"{n}.npy") for n in ("ids", "scores", "counts", "queries", "rows")})
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    a, b = runs
    assert a["ids"].dtype == np.float64 and a["scores"].dtype == np.float32 and a["queries"].dtype == np.float32
    assert a["ids"].shape == a["scores"].shape == (1024, 10) and a["counts"].shape == (1024,) and a["queries"].shape == (1024, 960)
    assert (a["counts"] == 10).all()
    for n in a:
        assert np.array_equal(a[n], b[n], equal_nan=(n == "scores")), n
