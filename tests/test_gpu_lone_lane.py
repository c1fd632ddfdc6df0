"""Lone lanes of the K1 host leg on the device (reflow_amd/csrc/host_leg.h,
DESIGN.md §5 "Lone lanes"): hybrid plans made with RF_SHA_LONE=1 and =2 on 2
and on 16 host threads, over files whose lengths straddle the copy ring of a
lone lane (four 16 MiB buffers over two streams) and a few 4 KiB files for the
GPU legs; again with RF_SHA_PREFIX_PRECLAIM=1, so that the lone rule and the
prefix hand-over meet; and RF_SHA_LONE=0, which plans and hashes as the library
did before lone lanes.  Every digest is checked against hashlib."""
import hashlib

import numpy as np
import pytest

from reflow_amd import capi
from reflow_amd.workloads import MiB, arena_layout

pytestmark = pytest.mark.gpu

C = 16 * MiB  # host_chunk_bytes()
BIG = [C - 1, C, C + 1, 2 * C + 65, 3 * C + 63, 4 * C, 5 * C + 64]  # 4 chunks: the ring wraps
SMALL = [4096] * 24
LENS = np.array(BIG + SMALL, dtype=np.uint64)


@pytest.fixture(scope="module")
def files():
    """The bytes and their hashlib digests, made once."""
    offs, total = arena_layout(LENS)
    host = np.frombuffer(np.random.default_rng(0x10BE).bytes(int(total)), dtype=np.uint8)
    want = [hashlib.sha256(host[int(o):int(o) + int(n)].tobytes()).digest() for o, n in zip(offs, LENS)]
    return offs, host, want


@pytest.fixture(scope="module", params=[2, 16])
def dev(request, files):
    offs, host, want = files
    c = capi.Context(0, host_threads=request.param)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    arena, out = c.upload(host), c.alloc(32 * len(LENS))
    yield c, arena, out
    arena.free()
    out.free()
    c.close()


def _digests(c, out):
    c.sync()
    got = out.to_numpy(count=32 * len(LENS)).reshape(-1, 32)
    return [got[i].tobytes() for i in range(len(LENS))]


def _run(dev, files, runs=2):
    """A default (hybrid) plan under the environment as it stands: its split,
    its lone count, and the digests of every run against hashlib."""
    c, arena, out = dev
    offs, _, want = files
    plan = c.sha_plan(offs, LENS, 0)
    st, ps = plan.stats(), plan.prefix_stats()
    for _ in range(runs):
        out.copy_from(np.zeros(32 * len(LENS), np.uint8))
        plan.run(arena.ptr, out.ptr)
        assert _digests(c, out) == want
        r = plan.prefix_stats()
        assert r.taken + r.missed == r.n_prefixed and r.skipped_bytes <= r.planned_bytes
    plan.close()
    return (int(st.n_host), int(st.n_solo), int(ps.n_prefixed)), int(ps.n_lone)


@pytest.mark.parametrize("lone", [1, 2])
@pytest.mark.parametrize("preclaim", [False, True])
def test_forced_lone_lanes(dev, files, monkeypatch, lone, preclaim):
    monkeypatch.setenv("RF_SHA_LONE", str(lone))
    if preclaim:
        monkeypatch.setenv("RF_SHA_PREFIX_PRECLAIM", "1")
    split, n_lone = _run(dev, files)
    assert split[0] == len(BIG), split  # the big files are the host leg's
    assert n_lone == lone


def test_lone_off_is_the_plan_as_it_was(dev, files, monkeypatch):
    """RF_SHA_LONE=0: no lone message, and the split the library made of this
    set before lone lanes (the 7 big files on the host leg, the 24 small ones
    on duo waves: measured on that library on 2 and on 16 threads,
    profiles/lone_lane/README.md).  The unset environment may choose lone
    lanes; its digests are the same."""
    monkeypatch.setenv("RF_SHA_LONE", "0")
    split, n_lone = _run(dev, files)
    assert n_lone == 0 and split[:2] == (len(BIG), len(SMALL)), split
    monkeypatch.delenv("RF_SHA_LONE")
    split2, n_lone2 = _run(dev, files, runs=1)
    assert split2[0] == len(BIG) and 0 <= n_lone2 <= len(BIG)


def test_flags_that_rule_lone_lanes_out(dev, files, monkeypatch):
    """All-host, no-host and one-lane-chain plans never have a lone message,
    whatever RF_SHA_LONE says."""
    c, arena, out = dev
    offs, _, want = files
    monkeypatch.setenv("RF_SHA_LONE", "2")
    for flags in (capi.RF_SHA_ALL_HOST, capi.RF_SHA_NO_HOST, capi.RF_SHA_ONE_LANE_CHAIN):
        plan = c.sha_plan(offs, LENS, flags)
        assert plan.prefix_stats().n_lone == 0, flags
        if flags == capi.RF_SHA_ALL_HOST:
            out.copy_from(np.zeros(32 * len(LENS), np.uint8))
            plan.run(arena.ptr, out.ptr)
            assert _digests(c, out) == want
        plan.close()
