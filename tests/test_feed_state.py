"""The change feed's poll-mode decision without a GPU
(tests/cpp/feed_state_test.cpp over reflow_amd/csrc/feed_state.cpp alone): every
sequence of at most 4 events after an open against the table written out
below.  The program is built by the host compiler alone and run twice: plain,
and under AddressSanitizer + UBSan.

Events: S input slots set, P one whole plain incremental step, F full
recompute, W any other slot write (adopt, a captured-graph step, part of a
step), Q poll.  Modes: L listed with the step's candidates, l listed with
none (only what earlier polls left pending), s scan."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "feed_state_test")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

# What has happened since the last poll (or the open) -> what each event makes
# of it.  clean: nothing; marked: slots set, no step yet; stepped: zero or
# more set_slots, then exactly one plain step, nothing after; dirty: the rest.
NEXT = {
    "clean":   {"S": "marked", "P": "stepped", "F": "dirty", "W": "dirty"},
    "marked":  {"S": "marked", "P": "stepped", "F": "dirty", "W": "dirty"},
    "stepped": {"S": "dirty",  "P": "dirty",   "F": "dirty", "W": "dirty"},
    "dirty":   {"S": "dirty",  "P": "dirty",   "F": "dirty", "W": "dirty"},
}
# The mode of a poll made in each state (the mark kernels hash slot-fused
# chains at once, so slots set without a step already moved job outputs).
POLL = {"clean": "l", "marked": "s", "stepped": "L", "dirty": "s"}


def expected(seq, force=False):
    state, modes = "clean", ""
    for e in seq + "Q":
        if e == "Q":
            modes += "s" if force else POLL[state]
            state = "clean"
        else:
            state = NEXT[state][e]
    return modes


@pytest.fixture(scope="module")
def bins():
    b = subprocess.run(["make", "-C", CSRC, "feed_state_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["PASS", ""]
    return dict(ln.split() for ln in lines[:-2])


@pytest.mark.parametrize("build", ["plain", "asan"])
@pytest.mark.parametrize("force", [False, True])
def test_every_sequence_up_to_four_events(bins, build, force):
    got = _run(bins[build], ["force"] if force else [])
    seqs = ["".join(t) for n in range(5) for t in itertools.product("SPFWQ", repeat=n)]
    assert len(seqs) == 781 and len(got) == 781
    bad = {s: (got.get(s or "-"), expected(s, force)) for s in seqs if got.get(s or "-") != expected(s, force)}
    assert not bad, dict(list(bad.items())[:10])


def test_the_cases_that_must_come_out_right(bins):
    got = _run(bins["plain"], [])
    assert got["P"] == "L" and got["SP"] == "L" and got["SSSP"] == "L"   # one plain step: listed
    assert got["QSP"] == "lL" and got["SPQ"] == "Ll"                     # ... after a poll too; then nothing left
    assert got["PP"] == "s" and got["SPSP"] == "s"                       # two steps
    assert got["SF"] == "s" and got["F"] == "s" and got["PF"] == "s"     # a full recompute
    assert got["W"] == "s" and got["PW"] == "s" and got["WP"] == "s"     # an adopt / a captured step
    assert got["PS"] == "s" and got["SPS"] == "s"                        # set_slots after the step
    assert got["S"] == "s"                                               # slots set, not stepped yet
    assert got["-"] == "l" and got["Q"] == "ll" and got["FQ"] == "sl"    # nothing since: no candidates
    assert got["FQSP"] == "sL"                                           # a scan poll clears the slate
