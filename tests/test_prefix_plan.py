"""The K1 prefix hand-over on the host, without a GPU (tests/cpp/prefix_plan_test.cpp):
the planner's schedule model (reflow_amd/csrc/host_sched.cpp) on configs[1]'s
sizes, and host_leg_run resuming from chaining values -- flags set, unset and
mixed, at the padding edges and the 64-block edges of the duo's double buffer
-- every digest against hashlib.  The program is built by the host compiler
alone and run twice: plain, and under AddressSanitizer + UBSan."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from reflow_amd.workloads import GiB, MiB, c2_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "prefix_plan_test")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def bins():
    b = subprocess.run(["make", "-C", CSRC, "prefix_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_schedule_model_on_configs1(bins, build, tmp_path):
    """The host list of configs[1] -- its 108 largest files, the ones the
    planner hands the 16 x 2 lanes -- at the host leg's measured rates
    (1.63 GB/s a lane beside its partner, 2.4 GB/s alone) and the duo's
    1.13 us a block: no prefix for the first threads x ways files, none past
    len / 64, prefixes monotone in start time (the program checks these and
    more for every run), and the bytes moved off the host as modelled when the
    hand-over was proposed: 3.43 GB at alpha 0.8, 3.85 GB at 0.9, +-0.2 GB,
    each with a shorter makespan than without prefixes."""
    lens = np.sort(c2_sizes(total_bytes=64 * GiB, seed=0x5EED0002))[::-1][:108]
    p = tmp_path / "lens.txt"
    p.write_text("\n".join(str(int(x)) for x in lens) + "\n")
    out = _run(bins[build], ["model", str(p)])
    assert out.strip().splitlines()[-1] == "PASS"
    fig = {}
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "alpha":
            fig[float(w[1])] = (float(w[3]), float(w[5]))
    print(fig)
    assert abs(fig[0.0][0] - 1.305) < 0.01  # the measured host leg: 1.30-1.32 s
    assert abs(fig[0.8][1] / 1e9 - 3.4) <= 0.2
    assert abs(fig[0.9][1] / 1e9 - 3.85) <= 0.2
    assert fig[0.8][0] < fig[0.0][0] and fig[0.9][0] < fig[0.0][0]


def _leg_case():
    """Messages of 129 whole blocks + r bytes for every padding edge r, each
    with every prefix edge, and one that crosses the leg's 8 MiB chunk after a
    resumed start."""
    lens, pfx = [], []
    for r in (0, 1, 55, 56, 63):
        n = 129 * 64 + r
        for pb in (1, 63, 64, 65, n // 64):
            lens.append(n)
            pfx.append(pb)
    for pb in (1, 3):
        lens.append(9 * MiB + 197)
        pfx.append(pb)
    lens += [0, 64, 128 + 55]  # every byte a prefix; and messages without one
    pfx += [0, 1, 2]
    lens += [5000, 64 * 200]
    pfx += [0, 0]
    return lens, pfx


@pytest.fixture(scope="module")
def leg_files(tmp_path_factory):
    lens, pfx = _leg_case()
    rng = np.random.default_rng(11)
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += (n + 15) // 16 * 16
    arena = rng.integers(0, 256, size=max(pos, 16), dtype=np.uint8)
    d = tmp_path_factory.mktemp("prefix_leg")
    arena.tofile(d / "arena.bin")
    want = [hashlib.sha256(arena[o:o + n].tobytes()).hexdigest() for o, n in zip(offs, lens)]
    tasks = {}
    for name, ready in (("set", lambda i: 1), ("unset", lambda i: 0), ("mixed", lambda i: i % 2)):
        t = d / ("tasks_%s.txt" % name)
        t.write_text("".join("%d %d %d %d\n" % (o, n, pb, ready(i))
                             for i, (o, n, pb) in enumerate(zip(offs, lens, pfx))))
        tasks[name] = str(t)
    return str(d / "arena.bin"), tasks, want


@pytest.mark.parametrize("build", ["plain", "asan"])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("flags", ["set", "unset", "mixed"])
def test_host_leg_resumes_from_chaining_values(bins, leg_files, build, threads, flags):
    """host_leg_run from host memory and through its chunked copy path (the
    program stands in for the D2H calls): a set flag resumes from the chaining
    value at byte 64 x prefix, an unset one hashes from byte 0 and never reads
    the value (it is junk there); the program checks the taken / missed /
    skipped counters, the digests are checked here against hashlib."""
    arena, tasks, want = leg_files
    for where in ("host", "device"):
        out = _run(bins[build], ["leg", arena, tasks[flags], str(threads), where])
        if out.strip() == "SKIP":
            pytest.skip("no SHA extensions on this CPU")
        assert out.split() == want, where
