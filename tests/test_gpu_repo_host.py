"""Runs tests/cpp/repo_mirror_test: the repository index through the C++ host
mirror (include/reflow_host.hpp RepoIndex) on the device --
TestCacheLookupMissing's shape, Put's first-wins rule, TestGC's objects
collected with the GcLiveset's filter, and random values and deps -- against
missing() / NeedTransfer worked out in the test program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "repo_mirror_test")


def test_repo_mirror_test_built_and_linked():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True).stdout
    assert "libreflow_hip.so" in out and "not found" not in out.split("libreflow_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_repo_index_through_the_host_mirror():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "PASS"
