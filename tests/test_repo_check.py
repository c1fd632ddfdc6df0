"""The repository index without a GPU: its host-only parts
(tests/cpp/repo_check_test.cpp over reflow_amd/csrc/repo_check.cpp, built by
the host compiler and run plain and under AddressSanitizer + UBSan), and the
entry points' argument checks, constants and struct layouts against
include/reflow_hip.h."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from reflow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "repo_check_test")
HEADER = os.path.join(ROOT, "include", "reflow_hip.h")


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "repo_check_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_repo_check_program(bins, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]


def test_entry_points_refuse_null_arguments():
    L = capi.lib()
    out = ctypes.c_void_p()
    o = capi.RepoMissingOut()
    calls = [
        lambda: L.rf_repo_new(None, 0, ctypes.byref(out)),
        lambda: L.rf_repo_new(None, 0, None),
        lambda: L.rf_repo_put(None, None, None, 0, None),
        lambda: L.rf_repo_put_device(None, None, None, 0, None, None),
        lambda: L.rf_repo_remove(None, None, 0, None),
        lambda: L.rf_repo_remove_device(None, None, 0, None, None),
        lambda: L.rf_repo_stat(None, None, 0, None),
        lambda: L.rf_repo_stat_device(None, None, 0, None, None),
        lambda: L.rf_repo_collect(None, None, None, None, None),
        lambda: L.rf_repo_stats_get(None, None, 0),
        lambda: L.rf_repo_missing(None, None, 0, None, None, ctypes.byref(o)),
        lambda: L.rf_repo_missing(None, None, 0, None, None, None),
        lambda: L.rf_repo_missing_device(None, None, 0, None, None, 0, ctypes.byref(o), None),
        lambda: L.rf_repo_need_transfer(None, None, None, 0, ctypes.byref(o)),
        lambda: L.rf_repo_need_transfer_device(None, None, None, 0, ctypes.byref(o), None),
    ]
    for i, call in enumerate(calls):
        assert call() == capi.RF_EINVAL, i
        assert len(L.rf_last_error()) > 0, i
    L.rf_repo_destroy(None)  # a no-op, like the other destroy calls


def _header_defines():
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(RF_REPO_\w+)\s+(\d+)u?\b", text)}


def _layout(struct, fields):
    src = ('#include <cstdio>\n#include <cstddef>\n#include "reflow_hip.h"\nint main() { printf("%%zu", '
           'sizeof(%s));\n' % struct +
           "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "}\n")
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "s.cpp"), os.path.join(tmp, "s")
        open(cpp, "w").write(src)
        subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), cpp, "-o", exe], check=True, timeout=120)
        return [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]


def test_constants_and_layouts_match_the_header():
    d = _header_defines()
    names = ["RF_REPO_MAX_ROWS", "RF_REPO_MIN_SLOTS", "RF_REPO_LIST_TILE"]
    assert sorted(d) == sorted(names)
    for name in names:
        assert getattr(capi, name) == d[name], name
    assert d["RF_REPO_MAX_ROWS"] == 1 << 30
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for struct, S in (("rf_repo_stats", capi.RepoStats), ("rf_repo_missing_out", capi.RepoMissingOut)):
        fields = [f[0] for f in S._fields_]
        assert _layout(struct, fields) == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields], struct
    assert [f[0] for f in capi.RepoStats._fields_] == ["objects", "bytes", "tombstones", "capacity", "rebuilds",
                                                       "device_bytes", "last_rows", "last_files", "last_missing"]
    assert [f[0] for f in capi.RepoMissingOut._fields_] == ["n_files", "n_missing", "missing_bytes", "status", "cap",
                                                            "miss_ptr", "miss_rows", "miss_ids32", "miss_sizes",
                                                            "n_listed"]
