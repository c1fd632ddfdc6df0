"""K1 checkpointed prefix hand-over on the device: a prefix wave of
k1_sha256_duo leaves its chaining value in host memory every
RF_SHA_PREFIX_CKPT blocks and at its cap, and stops at the first of these
after the host has claimed the file (reflow_amd/csrc/prefix_record.h,
host_leg.h).  Caps are forced through rf_sha_plan_set_prefixes
on messages whose whole blocks sit on and around the duo's 64-block chunk
edges, with the interval at one, two and three chunks:

  WAIT               every wave reaches its cap: the last record is the cap's
  WAIT + PRECLAIM    every file is claimed before the launch, so every wave
                     stops at its first record: this pins the chaining values
                     taken inside the chain at the first, second and third
                     chunk boundary
  RACE               the production behaviour: whatever the host finds

Every digest is checked against the oracle's SHA-256."""
import numpy as np
import pytest

from reflow_amd import capi
from reflow_amd.workloads import MiB

from test_gpu_prefix_handover import GenSet, HostSet, _want_stream

pytestmark = pytest.mark.gpu

RS = (0, 1, 55, 56, 63)
BLOCKS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4097)
BIG = 9 * MiB + 197  # 147,459 whole blocks
BIG2 = 17 * MiB + 197  # the host's 16 MiB chunk edge falls inside its suffix after a resumed start
LENS = [64 * b + RS[i % len(RS)] for i, b in enumerate(BLOCKS)] + [BIG, BIG2]
CAPS = (1, 63, 64, 65, 128, 129, None)  # None: every whole block
INTERVALS = (64, 128, 192)


@pytest.fixture(scope="module", params=[1, 3])
def ctx(request):
    c = capi.Context(0, host_threads=request.param)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    yield c
    c.close()


@pytest.fixture(scope="module")
def msgs(ctx, oracle):
    assert [int(n) // 64 for n in LENS] == list(BLOCKS) + [147459, 278531]
    hs = HostSet(ctx, oracle, LENS, 0x6B)
    yield hs
    hs.free()


def _runs(ctx, hs, monkeypatch, interval, mode, preclaim=False, reps=1):
    """One forced plan per cap; yields (stats, caps in host order) per run."""
    monkeypatch.setenv("RF_SHA_PREFIX_CKPT", str(interval))
    if preclaim:
        monkeypatch.setenv("RF_SHA_PREFIX_PRECLAIM", "1")
    for cap in CAPS:
        plan = ctx.sha_plan(hs.offs, hs.lens, capi.RF_SHA_ALL_HOST)
        assert plan.stats().n_host == len(LENS)
        pb = hs.prefixes([cap] * len(LENS))
        plan.set_prefixes(pb, mode)
        st = plan.prefix_stats()
        assert st.n_prefixed == len(LENS) and st.planned_bytes == 64 * int(pb.sum())
        for _ in range(reps):
            hs.out.copy_from(np.zeros(32 * len(LENS), np.uint8))
            plan.run(hs.arena.ptr, hs.out.ptr)
            assert hs.digests(ctx) == hs.want, (interval, cap, mode, preclaim)
            yield plan.prefix_stats(), pb
        plan.close()


@pytest.mark.parametrize("interval", INTERVALS)
def test_wait_takes_the_record_at_the_cap(ctx, msgs, monkeypatch, interval):
    for st, pb in _runs(ctx, msgs, monkeypatch, interval, capi.RF_PREFIX_WAIT):
        assert st.taken == len(LENS) and st.missed == 0
        assert st.skipped_bytes == st.planned_bytes == 64 * int(pb.sum())


@pytest.mark.parametrize("interval", INTERVALS)
def test_preclaimed_waves_stop_at_their_first_record(ctx, msgs, monkeypatch, interval):
    for st, pb in _runs(ctx, msgs, monkeypatch, interval, capi.RF_PREFIX_WAIT, preclaim=True):
        assert st.taken == len(LENS) and st.missed == 0
        assert st.skipped_bytes == 64 * int(np.minimum(pb, interval).sum()), (interval, pb)


@pytest.mark.parametrize("interval", INTERVALS)
def test_race_is_right_whatever_it_finds(ctx, msgs, monkeypatch, interval):
    for st, pb in _runs(ctx, msgs, monkeypatch, interval, capi.RF_PREFIX_RACE, reps=3):
        assert st.taken + st.missed == len(LENS)
        assert st.skipped_bytes <= st.planned_bytes


def test_default_plan_and_the_plans_without_prefixes(oracle, monkeypatch):
    """The eight 24 MiB files and 500 small ones of the planner test on one
    host thread: the default plan (the planner's caps, the default interval)
    equals the oracle with every prefixed file either taken or missed, and
    RF_SHA_NO_PREFIX and RF_SHA_PREFIX=0 plans carry no prefix and run as
    before."""
    c = capi.Context(0, host_threads=1)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    rng = np.random.default_rng(8)
    lens = np.concatenate([[24 * MiB + 64 * i + i for i in range(8)],
                           rng.integers(1, 64 * 1024, size=500)]).astype(np.uint64)
    ds = GenSet(c, lens, 0xABC)
    want = _want_stream(oracle, lens, 0xABC)
    plan = c.sha_plan(ds.offs, ds.lens, 0)
    n_pfx = plan.prefix_stats().n_prefixed
    assert n_pfx > 0
    for _ in range(2):
        assert (ds.run(c, plan) == want).all()
        r = plan.prefix_stats()
        print("default plan: %d prefixed, taken %d missed %d, %.1f of %.1f MiB"
              % (n_pfx, r.taken, r.missed, r.skipped_bytes / MiB, r.planned_bytes / MiB))
        assert r.taken + r.missed == n_pfx and r.skipped_bytes <= r.planned_bytes
    plan.close()
    plan = c.sha_plan(ds.offs, ds.lens, capi.RF_SHA_NO_PREFIX)
    assert plan.prefix_stats().n_prefixed == 0
    assert (ds.run(c, plan) == want).all()
    plan.close()
    monkeypatch.setenv("RF_SHA_PREFIX", "0")
    plan = c.sha_plan(ds.offs, ds.lens, 0)
    assert plan.prefix_stats().n_prefixed == 0
    assert (ds.run(c, plan) == want).all()
    plan.close()
    ds.free()
    c.close()
