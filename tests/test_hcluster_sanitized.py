"""The CPU clustering restatement under AddressSanitizer + UBSan: tests/test_hcluster_host.py in a child interpreter that loads the
sanitized builder (__graft_entry__.build_sanitized), as tests/test_closure_sanitized.py does for the closure."""
import os
import subprocess
import sys

from conftest import ROOT
from test_sanitizers import _san_env


def test_hcluster_restatement_under_asan_ubsan():
    env = _san_env()
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hcluster_host.py"), "-x", "-q", "-m", "not gpu",
                          "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "passed" in out.stdout and "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
