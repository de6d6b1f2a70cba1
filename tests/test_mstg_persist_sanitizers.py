"""tests/test_mstg_persist_host.py again with the AddressSanitizer + UBSan build of the CPU builder (the pattern of
tests/test_sanitizers.py): the `.mstg` framing parser and record checks see exact-size heap copies of every corrupted and
truncated file, so a read past the end of a buffer is a report, not a silent pass."""
import os
import subprocess
import sys

from conftest import ROOT
from test_sanitizers import _san_env


def test_mstg_file_checks_under_asan_ubsan():
    env = _san_env()
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_mstg_persist_host.py"), "-x", "-q",
                          "-m", "not gpu", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "passed" in out.stdout and "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
