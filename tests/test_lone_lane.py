"""Lone lanes of the K1 host leg on the host, without a GPU
(tests/cpp/lone_lane_test.cpp; DESIGN.md §5 "Lone lanes"): the schedule
model's lone rule on configs[1]'s host files, and host_leg_run with lone flags
in host memory and through the copy ring.  The program is built by the host
compiler alone and run as a plain executable: plain, under ASan + UBSan, and
under ThreadSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from reflow_amd.workloads import GiB, c2_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "lone_lane_test")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lone_lane", "sched_before_lone.txt")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

BUILDS = ["plain", "asan", "tsan"]


@pytest.fixture(scope="module")
def bins():
    b = subprocess.run(["make", "-C", CSRC, "lone_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan", "tsan": BIN + "_tsan"}


def _run(exe, args, **env):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
             UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("RF_HOST_CHUNK_MB", "RF_HOST_WAYS", "RF_HOST_LEG_TIMING"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def lens_file(tmp_path_factory):
    """configs[1]'s host files: the 111 largest, largest first."""
    lens = np.sort(c2_sizes(total_bytes=64 * GiB, seed=0x5EED0002))[::-1][:111]
    p = tmp_path_factory.mktemp("lone") / "lens.txt"
    p.write_text("\n".join(str(int(x)) for x in lens) + "\n")
    return str(p)


@pytest.mark.parametrize("build", BUILDS)
def test_model_on_configs1(bins, build, lens_file):
    """At DESIGN's rates (2.44 / 1.79 GB/s a lane, link 52 and 53.5 GB/s, duo
    1.13 us a block) lone = 0 gives, to the bit, what the model gave before it
    knew lone lanes (tests/golden/lone_lane/sched_before_lone.txt: makespan,
    skipped bytes and every message's start and prefix for three parameter
    sets, written by the model as it was).  With the link off the
    thread-bound end falls strictly from lone = 0 to lone = 1.  The program
    itself checks, for lone = 0..8, 16, 17, 40, n and n + 5 on these files and
    for 1..64 threads x 1..4 ways on a shorter list, that every message is
    claimed exactly once, that no two overlap in a lane and that nothing is
    claimed on a thread while it holds a lone message, and that ways = 1
    makes lone a no-op."""
    out = _run(bins[build], ["model", lens_file])
    assert out.strip().splitlines()[-1] == "PASS"
    got = [ln for ln in out.splitlines() if ln[:2] in ("S ", "M ")]
    with open(GOLDEN) as f:
        assert got == f.read().splitlines()
    table = {}
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "T":
            table[int(w[1])] = tuple(float(x) for x in w[2:5])
    print("lone -> thread-bound end, makespan at 52 GB/s, at 53.5 GB/s:", table)
    assert table[1][0] < table[0][0]


@pytest.mark.parametrize("build", BUILDS)
def test_host_resident_leg_with_lone_flags(bins, build):
    """host_leg_run from host memory on 2 threads with lone flags, at the
    product's chunk (16 MiB) and lanes (2): messages of 0, 1, 55, 56, 64,
    2 chunks - 1, 2 chunks and 2 chunks + 65 bytes, every digest against
    host_sha run serially (the program compares)."""
    cases = [(o, k) for o in ("up", "down") for k in ("0", "1", "2", "8", "alt")]
    if build != "plain":  # the sanitized builds hash slowly: the two that mix lone and ordinary messages
        cases = [("down", "2"), ("up", "alt")]
    for order, lone in cases:
        out = _run(bins[build], ["leg", "2", "host", order, lone])
        if out.strip() == "SKIP":
            pytest.skip("no SHA extensions on this CPU")
        assert out.strip().splitlines()[-1] == "PASS", (order, lone)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("copies", ["eager", "lazy"])
def test_copy_ring(bins, build, copies):
    """The same, through the chunked copy path over the program's stand-ins
    for the HIP calls, with messages that straddle the ring (1 chunk - 1 ..
    7 chunks + 1; 1 MiB chunks): eager copies spoil a buffer that is queued
    into too early, lazy ones leave a chunk stale that is hashed before its
    stream was waited for, and a second copy on a stream that still holds one
    fails the run.  One thread whose messages are all lone never has two
    messages at once, so two copies in flight are the ring's."""
    cases = [(1, 2, "down", "99"), (2, 2, "down", "2"), (2, 2, "up", "alt"), (2, 3, "down", "alt"),
             (2, 1, "down", "2")]
    if build == "plain":
        cases += [(1, 2, "down", "1"), (3, 2, "up", "99"), (1, 4, "up", "alt"), (2, 2, "down", "0")]
    for threads, ways, order, lone in cases:
        out = _run(bins[build], ["leg", str(threads), copies, order, lone], RF_HOST_CHUNK_MB="1",
                   RF_HOST_WAYS=str(ways))
        if out.strip() == "SKIP":
            pytest.skip("no SHA extensions on this CPU")
        assert out.strip().splitlines()[-1] == "PASS", (threads, ways, order, lone)
        inflight = int(out.split("max_inflight")[1].split()[0])
        assert inflight <= max(2, ways)
        if (threads, ways, lone) == (1, 2, "99"):
            assert inflight == 2
        if ways == 1:
            assert inflight == 1
