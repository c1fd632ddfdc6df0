"""Runs tests/cpp/phys_mirror_test: reflow::PhysicalKeys of the C++ host mirror
(include/reflow_host.hpp) on the device -- values from Fileset objects and from
an unmarshalled forest, the consumers' physical keys, a replaced and a cleared
value, the value digests."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "phys_mirror_test")


def test_phys_mirror_test_built_and_linked():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True).stdout
    assert "libreflow_hip.so" in out and "not found" not in out.split("libreflow_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_physical_keys_through_the_host_mirror():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "PASS"
