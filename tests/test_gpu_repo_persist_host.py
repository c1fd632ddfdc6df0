"""Runs tests/cpp/repo_persist_test: the repository index read back through
the C++ host mirror (include/reflow_host.hpp RepoIndex) on the device -- List,
CollectList with a GcLiveset's filter on TestGC's objects and with a nil
liveset, Compact, and Save / Restore -- against a std::map in the test program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "repo_persist_test")


def test_repo_persist_test_built_and_linked():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True).stdout
    assert "libreflow_hip.so" in out and "not found" not in out.split("libreflow_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_repo_listing_and_persistence_through_the_host_mirror(tmp_path):
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "PASS"
