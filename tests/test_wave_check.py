"""The evaluation waves without a GPU: the consumer CSR
(tests/cpp/wave_check_test.cpp over reflow_amd/csrc/wave_check.cpp alone,
built by the host compiler and run plain and under AddressSanitizer + UBSan),
rf_eval_wave_consumers through the library with its refusals, and the entry
points' argument checks, constants and stats layout against
include/reflow_hip.h."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import wave_model as W
from reflow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "wave_check_test")
HEADER = os.path.join(ROOT, "include", "reflow_hip.h")


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "wave_check_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_wave_check_program(bins, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]


def _csr(dep_lists):
    ptr = np.zeros(len(dep_lists) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(d) for d in dep_lists])
    return ptr, np.array([x for d in dep_lists for x in d], dtype=np.uint32)


def _consumers(dep_lists):
    cp, co = capi.eval_wave_consumers(*_csr(dep_lists))
    assert cp[0] == 0 and cp[-1] == len(co) == sum(len(d) for d in dep_lists)
    return [co[int(cp[i]):int(cp[i + 1])].tolist() for i in range(len(dep_lists))]


def _refused(dep_ptr, deps):
    with pytest.raises(capi.RfError) as ei:
        capi.eval_wave_consumers(dep_ptr, deps)
    assert ei.value.code == capi.RF_EINVAL
    return str(ei.value)


def test_consumers_through_the_library():
    cp, co = capi.eval_wave_consumers(np.zeros(0, np.uint64), np.zeros(0, np.uint32))  # empty
    assert cp.tolist() == [0] and len(co) == 0
    assert _consumers([[]]) == [[]]                                                        # n = 1
    chain = [[i + 1] for i in range(99)] + [[]]
    assert _consumers(chain) == [[]] + [[i] for i in range(99)]
    assert _consumers([[1, 2, 2], [3], [3], [], []]) == [[], [0], [0, 0], [1, 2], []]      # a dep listed twice
    for k in (0, 63, 64, 65, 130):                                                         # k consumers of one node
        d = k // 2
        got = _consumers([[] if i == d else [d] for i in range(k + 1)])
        assert got[d] == [i for i in range(k + 1) if i != d] and sum(map(len, got)) == k
    rng = np.random.default_rng(3)
    for t in range(20):  # random DAGs against the naive inversion; ascending within a node
        n = int(rng.integers(1, 200))
        if t % 2:
            lists = [list(rng.integers(i + 1, n, size=rng.integers(0, 5))) if i + 1 < n else [] for i in range(n)]
        else:
            lists = [list(rng.integers(0, i, size=rng.integers(0, 5))) if i else [] for i in range(n)]
        got = _consumers(lists)
        assert got == W.consumers(lists) and all(g == sorted(g) for g in got)
    # the refusals
    assert "cycle" in _refused(*_csr([[0]]))
    assert "cycle" in _refused(*_csr([[1], [2], [1]]))
    assert "out of range" in _refused(*_csr([[2], []]))
    assert "monotone" in _refused(np.array([0, 1, 0], np.uint64), np.array([1], np.uint32))
    assert "dep_ptr[0]" in _refused(np.array([1, 1], np.uint64), np.array([0], np.uint32))
    L = capi.lib()
    ptr, deps = _csr([[1], []])
    cp, co = np.full(3, 9, np.uint64), np.full(1, 9, np.uint32)
    assert L.rf_eval_wave_consumers(2, None, deps.ctypes.data, cp.ctypes.data, co.ctypes.data) == capi.RF_EINVAL
    assert L.rf_eval_wave_consumers(2, ptr.ctypes.data, None, cp.ctypes.data, co.ctypes.data) == capi.RF_EINVAL
    assert L.rf_eval_wave_consumers(2, ptr.ctypes.data, deps.ctypes.data, None, co.ctypes.data) == capi.RF_EINVAL
    assert L.rf_eval_wave_consumers(2, ptr.ctypes.data, deps.ctypes.data, cp.ctypes.data, None) == capi.RF_EINVAL
    assert cp.tolist() == [9, 9, 9] and co.tolist() == [9]  # untouched
    assert L.rf_eval_wave_consumers(2, ptr.ctypes.data, deps.ctypes.data, cp.ctypes.data, co.ctypes.data) == capi.RF_OK
    assert cp.tolist() == [0, 0, 1] and co.tolist() == [0]


def test_entry_points_refuse_null_arguments():
    L = capi.lib()
    out = ctypes.c_void_p()
    n8 = ctypes.c_uint64()
    calls = [
        lambda: L.rf_eval_wave_open(None, 0, None, None, None, None, None, ctypes.byref(out)),
        lambda: L.rf_eval_wave_open(None, 0, None, None, None, None, None, None),
        lambda: L.rf_eval_wave_consumers(1, None, None, None, None),
        lambda: L.rf_eval_wave_set_flags(None, None, None, 0),
        lambda: L.rf_eval_wave_begin(None, None, 0, 0, None, None, None, None, 0, None),
        lambda: L.rf_eval_wave_begin_host(None, None, 0, 0, None, None, None, 0),
        lambda: L.rf_eval_wave_begin_states(None, None, 0, None),
        lambda: L.rf_eval_wave_step(None, None, 0, None, None, None, None, 0, None),
        lambda: L.rf_eval_wave_step_host(None, None, 0, None, None, None, 0),
        lambda: L.rf_eval_wave_reject(None, None, 0),
        lambda: L.rf_eval_wave_states(None, None),
        lambda: L.rf_eval_wave_states_device(None, None),
        lambda: L.rf_eval_wave_list(None, capi.RF_PLAN_HIT, capi.RF_WAVE_ALL, 0, None, None, None, None,
                                    ctypes.byref(n8)),
        lambda: L.rf_eval_wave_list_device(None, capi.RF_PLAN_HIT, capi.RF_WAVE_LAST, 0, None, None, None, None,
                                           None, None),
        lambda: L.rf_eval_wave_stats_get(None, None, 0),
    ]
    for i, call in enumerate(calls):
        assert call() == capi.RF_EINVAL, i
        assert len(L.rf_last_error()) > 0, i
    L.rf_eval_wave_close(None)  # a no-op, like the other destroy calls


def test_constants_and_stats_layout_match_the_header():
    text = open(HEADER).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(RF_WAVE_\w+)\s+(\d+)u?\b", text)}
    assert d == {"RF_WAVE_ALL": capi.RF_WAVE_ALL, "RF_WAVE_LAST": capi.RF_WAVE_LAST}
    assert (W.ALL, W.LAST) == (capi.RF_WAVE_ALL, capi.RF_WAVE_LAST)
    assert (W.NONE, W.BOTTOMUP, W.TOPDOWN) == (capi.RF_WAVE_MODE_NONE, capi.RF_WAVE_MODE_BOTTOMUP,
                                               capi.RF_WAVE_MODE_TOPDOWN)
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    fields = ["n_deps", "depth", "mode", "waves", "last_wave", "rounds", "round_batch", "wave_lanes", "list_tile",
              "counts", "looked_up", "keys_probed", "keys_filtered", "device_bytes"]
    src = ('#include <cstdio>\n#include <cstddef>\n#include "reflow_hip.h"\nint main() { printf("%zu", '
           'sizeof(rf_eval_wave_stats));\n' +
           "".join('printf(" %%zu", offsetof(rf_eval_wave_stats, %s));\n' % f for f in fields) + "}\n")
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "s.cpp"), os.path.join(tmp, "s")
        open(cpp, "w").write(src)
        subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), cpp, "-o", exe], check=True, timeout=120)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = capi.EvalWaveStats
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
