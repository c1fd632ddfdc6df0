"""The GC liveset without a GPU: its host-only parts
(tests/cpp/live_check_test.cpp over reflow_amd/csrc/live_check.cpp, built by
the host compiler and run plain and under AddressSanitizer + UBSan),
rf_bloom_estimate through the library against the oracle's
estimate_parameters, and the entry points' argument checks, constants and
stats layout against include/reflow_hip.h."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import reflow_oracle as O
from reflow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "live_check_test")
HEADER = os.path.join(ROOT, "include", "reflow_hip.h")


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "live_check_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_live_check_program(bins, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]


def test_bloom_estimate_equals_the_oracle():
    for n in list(range(1, 20001)) + [10 ** 5, 10 ** 6, 10 ** 7]:
        assert capi.bloom_estimate(n, 0.001) == O.estimate_parameters(n, 0.001), n
    assert capi.bloom_estimate(1000, 0.001) == (14378, 10)
    assert capi.bloom_estimate(10 ** 8, 0.001) == (1437758757, 10)
    assert capi.bloom_estimate(500, 0.01) == O.estimate_parameters(500, 0.01)


@pytest.mark.parametrize("n,p", [(0, 0.001), (10, 0.0), (10, 1.0), (10, -1.0), (10, 1.5), (10, float("nan"))])
def test_bloom_estimate_refusals(n, p):
    with pytest.raises(capi.RfError) as ei:
        capi.bloom_estimate(n, p)
    assert ei.value.code == capi.RF_EINVAL and "bloom_estimate" in str(ei.value)


def test_entry_points_refuse_null_arguments():
    L = capi.lib()
    out = ctypes.c_void_p()
    n8 = ctypes.c_uint64()
    calls = [
        lambda: L.rf_bloom_estimate(10, 0.001, None, None),
        lambda: L.rf_liveset_open(None, 0, None, None, ctypes.byref(out)),
        lambda: L.rf_liveset_open(None, 0, None, None, None),
        lambda: L.rf_liveset_set_values(None, None, None, 0, None, None),
        lambda: L.rf_liveset_set_values_device(None, None, None, 0, None, None, None),
        lambda: L.rf_liveset_clear_values(None, None, 0),
        lambda: L.rf_liveset_run(None, None, 0, None, 0, None),
        lambda: L.rf_liveset_filter(None, ctypes.byref(out)),
        lambda: L.rf_liveset_filter(None, None),
        lambda: L.rf_liveset_states(None, None),
        lambda: L.rf_liveset_list(None, capi.RF_LIVE_VALUE, 0, None, ctypes.byref(n8)),
        lambda: L.rf_liveset_stats_get(None, None, 0),
    ]
    for i, call in enumerate(calls):
        assert call() == capi.RF_EINVAL, i
        assert len(L.rf_last_error()) > 0, i
    L.rf_liveset_close(None)  # a no-op, like the other destroy calls
    L.rf_bloom_destroy(None)


def _header_defines():
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(RF_LIVE_\w+)\s+(\d+)u?\b", text)}


def test_constants_and_stats_layout_match_the_header():
    d = _header_defines()
    names = ["RF_LIVE_UNSEEN", "RF_LIVE_WALKED", "RF_LIVE_VALUE", "RF_LIVE_MAX_ROWS", "RF_LIVE_LIST_TILE",
             "RF_LIVE_ROUND_BATCH"]
    assert sorted(d) == sorted(names)
    for name in names:
        assert getattr(capi, name) == d[name], name
    assert d["RF_LIVE_MAX_ROWS"] >= 1 << 30
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    fields = ["counts", "contributions", "nlive_est", "nlive", "livebytes", "maxlivebytes", "m", "k", "rounds",
              "changed", "arena_rows", "stale_rows", "device_bytes"]
    src = ('#include <cstdio>\n#include <cstddef>\n#include "reflow_hip.h"\nint main() { printf("%zu", '
           'sizeof(rf_liveset_stats));\n' +
           "".join('printf(" %%zu", offsetof(rf_liveset_stats, %s));\n' % f for f in fields) + "}\n")
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "s.cpp"), os.path.join(tmp, "s")
        open(cpp, "w").write(src)
        subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), cpp, "-o", exe], check=True, timeout=120)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = capi.LivesetStats
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
