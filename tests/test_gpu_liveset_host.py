"""Runs tests/cpp/live_mirror_test: the GC liveset through the C++ host mirror
(include/reflow_host.hpp GcLiveset) on the device -- TestGC's flow stage by
stage and one random graph -- against Eval.collect worked out in the test
program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "live_mirror_test")


def test_live_mirror_test_built_and_linked():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True).stdout
    assert "libreflow_hip.so" in out and "not found" not in out.split("libreflow_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_liveset_through_the_host_mirror():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "PASS"
