"""The evaluation plan without a GPU: the structural checks of its node graph
(tests/cpp/plan_check_test.cpp over reflow_amd/csrc/plan_check.cpp alone,
built by the host compiler and run plain and under AddressSanitizer + UBSan),
rf_eval_plan_check through the library, and the entry points' argument
checks, constants and stats layout against include/reflow_hip.h."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from reflow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "plan_check_test")
HEADER = os.path.join(ROOT, "include", "reflow_hip.h")


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "plan_check_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_plan_check_program(bins, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]


def _csr(dep_lists):
    ptr = np.zeros(len(dep_lists) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(d) for d in dep_lists])
    return ptr, np.array([x for d in dep_lists for x in d], dtype=np.uint32)


def _refused(dep_ptr, deps):
    with pytest.raises(capi.RfError) as ei:
        capi.eval_plan_check(dep_ptr, deps)
    assert ei.value.code == capi.RF_EINVAL and "eval_plan" in str(ei.value)
    return str(ei.value)


def test_check_through_the_library():
    assert capi.eval_plan_check(np.zeros(0, np.uint64), np.zeros(0, np.uint32)) == 0
    assert capi.eval_plan_check(np.zeros(1, np.uint64), np.zeros(0, np.uint32)) == 0
    assert capi.eval_plan_check(*_csr([[i + 1] for i in range(99)] + [[]])) == 100          # chain
    assert capi.eval_plan_check(*_csr([[1, 2, 2], [3], [3], [], []])) == 3                  # diamond, a dep twice
    assert "cycle" in _refused(*_csr([[0]]))                                                # self-loop
    assert "cycle" in _refused(*_csr([[1], [2], [1]]))                                      # 2-cycle
    assert "cycle" in _refused(*_csr([[(i + 1) % 3000] for i in range(3000)]))              # long cycle
    assert "out of range" in _refused(*_csr([[2], []]))
    assert "monotone" in _refused(np.array([0, 1, 0], np.uint64), np.array([1], np.uint32))
    assert "dep_ptr[0]" in _refused(np.array([1, 1], np.uint64), np.array([0], np.uint32))
    # random DAGs (deps point at higher ids) against a recursive depth
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = int(rng.integers(1, 200))
        lists = [list(rng.integers(i + 1, n, size=rng.integers(0, 4))) if i + 1 < n else [] for i in range(n)]
        depth = [0] * n
        for i in range(n - 1, -1, -1):
            depth[i] = 1 + max((depth[d] for d in lists[i]), default=0)
        assert capi.eval_plan_check(*_csr(lists)) == max(depth)
    # the depth output is optional
    ptr, deps = _csr([[1], []])
    assert capi.lib().rf_eval_plan_check(2, ptr.ctypes.data, deps.ctypes.data, None) == capi.RF_OK


def test_entry_points_refuse_null_arguments():
    L = capi.lib()
    out = ctypes.c_void_p()
    n8 = ctypes.c_uint64()
    calls = [
        lambda: L.rf_eval_plan_open(None, 0, None, None, None, None, None, ctypes.byref(out)),
        lambda: L.rf_eval_plan_open(None, 0, None, None, None, None, None, None),
        lambda: L.rf_eval_plan_check(1, None, None, None),
        lambda: L.rf_eval_plan_set_flags(None, None, None, 0),
        lambda: L.rf_eval_plan_run(None, None, 0, 0, None, None, None, None, 0, None),
        lambda: L.rf_eval_plan_run_host(None, None, 0, 0, None, None, None, 0),
        lambda: L.rf_eval_plan_reject(None, None, 0, None, None, None, None, 0, None),
        lambda: L.rf_eval_plan_reject_host(None, None, 0, None, None, None, 0),
        lambda: L.rf_eval_plan_states(None, None),
        lambda: L.rf_eval_plan_states_device(None, None),
        lambda: L.rf_eval_plan_list(None, capi.RF_PLAN_HIT, 0, None, None, None, None, ctypes.byref(n8)),
        lambda: L.rf_eval_plan_list_device(None, capi.RF_PLAN_HIT, 0, None, None, None, None, None, None),
        lambda: L.rf_eval_plan_stats_get(None, None, 0),
    ]
    for i, call in enumerate(calls):
        assert call() == capi.RF_EINVAL, i
        assert len(L.rf_last_error()) > 0, i
    L.rf_eval_plan_close(None)  # a no-op, like the other destroy calls


def _header_defines():
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(RF_PLAN_\w+)\s+(\d+)u?\b", text)}


def test_constants_and_stats_layout_match_the_header():
    d = _header_defines()
    names = ["RF_PLAN_F_CACHEABLE", "RF_PLAN_F_EXTERN", "RF_PLAN_F_INVALID", "RF_PLAN_F_DONE", "RF_PLAN_UNSEEN",
             "RF_PLAN_TODO", "RF_PLAN_READY", "RF_PLAN_HIT", "RF_PLAN_DONE", "RF_PLAN_MAX_KEYS"]
    assert sorted(d) == sorted(names)
    for name in names:
        assert getattr(capi, name) == d[name], name
    # the struct as the C compiler lays it out
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = ('#include <cstdio>\n#include <cstddef>\n#include "reflow_hip.h"\nint main() { printf("%zu %zu %zu %zu\\n", '
           'sizeof(rf_eval_plan_stats), offsetof(rf_eval_plan_stats, counts), '
           'offsetof(rf_eval_plan_stats, looked_up), offsetof(rf_eval_plan_stats, device_bytes)); }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "s.cpp"), os.path.join(tmp, "s")
        open(cpp, "w").write(src)
        subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), cpp, "-o", exe], check=True, timeout=120)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = capi.EvalPlanStats
    assert got == [ctypes.sizeof(S), S.counts.offset, S.looked_up.offset, S.device_bytes.offset]
