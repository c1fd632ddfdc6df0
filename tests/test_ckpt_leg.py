"""The checkpointed prefix hand-over on the host, without a GPU
(tests/cpp/ckpt_leg_test.cpp): host_leg_run claims files whose records
(reflow_amd/csrc/prefix_record.h) were prepared as a duo wave leaves them --
record numbers 0, 1, 2 and 7, block counts at the 64-block edges, at the cap
and at a cap that is no multiple of 64, the other slot junk, resumed starts
in front of the leg's chunk boundary (a 9 MiB and a 17 MiB message, for 8 and
16 MiB chunks), a prefix that is the whole message --
and the program checks every digest against host_sha256, the taken / missed /
skipped counters and the claimed words, and the retry rule as the pure
function it is.  Built by the host compiler alone and run twice: plain, and
under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "ckpt_leg_test")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def bins():
    b = subprocess.run(["make", "-C", CSRC, "ckpt_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("where", ["host", "device"])
def test_host_leg_resumes_from_records(bins, build, threads, where):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build], str(threads), where], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if r.stdout.strip() == "SKIP":
        pytest.skip("no SHA extensions on this CPU")
    assert r.stdout.strip() == "PASS"
