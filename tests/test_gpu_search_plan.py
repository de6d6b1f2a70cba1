"""The routes of the search plan on the GPU (rbq_host::plan_search behind rbq_debug_stage_resources): for the
grid of call shapes and forcing options of tools/route_dump.py, the workgroups and threads of every stage and the rank stage's
operands equal tests/golden/search_routes.jsonl, recorded from the commit before the plan existed (in route_dump's folded form:
equal lines are equal calls).  Nothing is launched."""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _route_dump():
    spec = importlib.util.spec_from_file_location("route_dump", os.path.join(ROOT, "tools", "route_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "search_routes.jsonl")) as f:
        return f.read().splitlines()


@pytest.mark.parametrize("i", [0, 1], ids=["d64_64_lists_1bit", "d256_4096_lists_7bit_kac"])
def test_routes_equal_the_golden(golden, i):
    rd = _route_dump()
    want = [l for l in golden if l.startswith('{"call":"%d/' % i)]
    assert len(want) == 1 + len(rd.FORCED)
    idx = rd.build(i)
    w = rd.Writer(rd.golden_row)
    ncalls = 0
    for key, per_nq in rd.routes(idx, i):
        w.add(key, per_nq)
        ncalls += sum(len(c) for c in per_nq.values())
    idx.close()
    assert ncalls == (1 + len(rd.FORCED)) * len(rd.NQ) * len(rd.TOP_K) * len(rd.NPROBE)
    wrong = [(g, l) for g, l in zip(want, w.lines) if g != l]
    assert not wrong, (len(wrong), wrong[:2])
