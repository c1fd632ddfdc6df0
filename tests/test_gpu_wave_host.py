"""Runs tests/cpp/wave_mirror_test: the evaluation waves through the C++ host
mirror (include/reflow_host.hpp EvalWave) on the device -- bottom-up from host
keys and from the Eval's graph, reject, refusals, set_flags, NoCacheExtern, a
liveset and the hand-over from an EvalPlan -- against the states Eval.todo +
Eval.lookup give by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "wave_mirror_test")


def test_wave_mirror_test_built_and_linked():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True).stdout
    assert "libreflow_hip.so" in out and "not found" not in out.split("libreflow_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_waves_through_the_host_mirror():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "PASS"
