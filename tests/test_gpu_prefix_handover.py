"""K1 prefix hand-over on the device: k1_sha256_duo hashes the first blocks of
host-leg messages and leaves their chaining values in host memory, the host
leg resumes from them (reflow_amd/csrc/host_sched.h, host_leg.h).  Prefixes
are forced through rf_sha_plan_set_prefixes at the duo's 64-block
double-buffer edges and the padding edges, in the three modes: WAIT (every
prefix taken), MISS (none), RACE (the production behaviour: whichever the
host finds).  Every digest is checked against the oracle's SHA-256."""
import os

import numpy as np
import pytest

from reflow_amd import capi
from reflow_amd.workloads import MiB, arena_layout

pytestmark = pytest.mark.gpu

RS = (0, 1, 55, 56, 63)
LENS12 = ([129 * 64 + r for r in RS] + [8192]) * 2
PREFIX_EDGES = (1, 63, 64, 65, 127, 128, 129, None)  # None: every whole block
BIG = 9 * MiB + 197  # the host's 8 MiB chunk boundary falls after a resumed start


class HostSet:
    """Messages of oracle.fill_stream bytes uploaded to an arena."""

    def __init__(self, ctx, oracle, lens, seed):
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64)
        self.offs, total = arena_layout(self.lens)
        host = np.zeros(max(int(total), 16), dtype=np.uint8)
        self.want = []
        for i, (o, n) in enumerate(zip(self.offs, self.lens)):
            m = oracle.fill_stream(seed ^ i, int(n))
            host[int(o):int(o) + int(n)] = np.frombuffer(m, np.uint8)
            self.want.append(oracle.sha256(m))
        self.arena = ctx.upload(host)
        self.out = ctx.alloc(32 * len(self.lens))
        # the plan's host order: blocks descending, stable
        nb = (self.lens.astype(np.int64) + 9 + 63) // 64
        self.order = np.argsort(-nb, kind="stable")

    def prefixes(self, per_message):
        """per-message prefix blocks (None: all whole blocks) -> host order."""
        pm = [int(n) // 64 if p is None else min(p, int(n) // 64) for p, n in zip(per_message, self.lens)]
        return np.array([pm[i] for i in self.order], dtype=np.uint64)

    def digests(self, ctx):
        ctx.sync()
        got = self.out.to_numpy(count=32 * len(self.lens)).reshape(-1, 32)
        return [got[i].tobytes() for i in range(len(self.lens))]

    def free(self):
        self.arena.free()
        self.out.free()


@pytest.fixture(scope="module", params=[1, 3])
def ctx(request):
    c = capi.Context(0, host_threads=request.param)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(ctx, oracle):
    a, b = HostSet(ctx, oracle, LENS12, 0x51), HostSet(ctx, oracle, [BIG], 0x77)
    yield a, b
    a.free()
    b.free()


def _forced_runs(sets):
    """(set, per-message prefixes): the twelve messages with every edge on
    every length (eight rotations), the big one with prefix 1 and 3."""
    twelve, big = sets
    for shift in range(len(PREFIX_EDGES)):
        yield twelve, [PREFIX_EDGES[(i + shift) % len(PREFIX_EDGES)] for i in range(len(LENS12))]
    yield big, [1]
    yield big, [3]


def _run_mode(ctx, sets, mode, reps=1):
    for hs, per_msg in _forced_runs(sets):
        plan = ctx.sha_plan(hs.offs, hs.lens, capi.RF_SHA_ALL_HOST)
        assert plan.stats().n_host == len(hs.lens) and plan.prefix_stats().n_prefixed == 0
        pb = hs.prefixes(per_msg)
        plan.set_prefixes(pb, mode)
        n_pfx = int((pb > 0).sum())
        assert plan.prefix_stats().n_prefixed == n_pfx and plan.prefix_stats().planned_bytes == 64 * int(pb.sum())
        for _ in range(reps):
            hs.out.copy_from(np.zeros(32 * len(hs.lens), np.uint8))
            plan.run(hs.arena.ptr, hs.out.ptr)
            assert hs.digests(ctx) == hs.want, (mode, per_msg)
            yield plan.prefix_stats(), n_pfx, pb
        plan.close()


def test_wait_mode_takes_every_prefix(ctx, sets):
    for st, n_pfx, pb in _run_mode(ctx, sets, capi.RF_PREFIX_WAIT):
        assert st.taken == n_pfx and st.missed == 0
        assert st.skipped_bytes == 64 * int(pb.sum())


def test_miss_mode_falls_back_everywhere(ctx, sets):
    for st, n_pfx, pb in _run_mode(ctx, sets, capi.RF_PREFIX_MISS):
        assert st.taken == 0 and st.missed == n_pfx and st.skipped_bytes == 0


def test_race_mode_is_right_either_way(ctx, sets):
    for st, n_pfx, pb in _run_mode(ctx, sets, capi.RF_PREFIX_RACE, reps=3):
        assert st.taken + st.missed == n_pfx  # no assertion on the split


def test_set_prefixes_refuses_a_prefix_past_the_data(ctx, sets):
    twelve, _ = sets
    plan = ctx.sha_plan(twelve.offs, twelve.lens, capi.RF_SHA_ALL_HOST)
    pb = twelve.prefixes([None] * len(LENS12))
    pb[0] += 1
    with pytest.raises(capi.RfError) as e:
        plan.set_prefixes(pb, capi.RF_PREFIX_WAIT)
    assert e.value.code == capi.RF_EINVAL
    plan.close()


# ---- the planner's own prefixes and the flags -------------------------------
def _want_stream(oracle, lens, seed):
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.zeros(32 * len(lens), dtype=np.uint8)
    oracle.lib().orc_stream_sha256_batch(seed, lens.ctypes.data, len(lens), out.ctypes.data, os.cpu_count() or 1)
    return out.reshape(-1, 32)


class GenSet:
    def __init__(self, ctx, lens, seed):
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64)
        self.offs, total = arena_layout(self.lens)
        self.arena = ctx.alloc(total)
        d_offs, d_lens = ctx.upload(self.offs), ctx.upload(self.lens)
        self.out = ctx.alloc(32 * len(self.lens))
        ctx.gen_fill(self.arena.ptr, d_offs.ptr, d_lens.ptr, len(self.lens), seed, total)
        ctx.sync()
        d_offs.free()
        d_lens.free()

    def run(self, ctx, plan):
        plan.run(self.arena.ptr, self.out.ptr)
        ctx.sync()
        return self.out.to_numpy(count=32 * len(self.lens)).reshape(-1, 32)

    def free(self):
        self.arena.free()
        self.out.free()


def test_flags_on_a_mixed_set(oracle):
    """The mixed set of test_hybrid_split_mixed_set under the default flags
    equals the oracle; RF_SHA_NO_PREFIX, RF_SHA_ALL_HOST and RF_SHA_NO_HOST
    plans carry no prefix."""
    c = capi.Context(0)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    rng = np.random.default_rng(5)
    lens = np.concatenate([[96 * MiB, 72 * MiB], rng.integers(1, 256 * 1024, size=3000)]).astype(np.uint64)
    ds = GenSet(c, lens, 99)
    want = _want_stream(oracle, lens, 99)
    plan = c.sha_plan(ds.offs, ds.lens, 0)
    assert (ds.run(c, plan) == want).all()
    st = plan.prefix_stats()
    assert st.taken + st.missed == st.n_prefixed
    plan.close()
    for flags in (capi.RF_SHA_NO_PREFIX, capi.RF_SHA_ALL_HOST, capi.RF_SHA_NO_HOST):
        plan = c.sha_plan(ds.offs, ds.lens, flags)
        assert plan.prefix_stats().n_prefixed == 0, flags
        plan.close()
    ds.free()
    c.close()


def test_planner_made_prefixes_one_thread(oracle):
    """One host thread (two lanes) and eight 24 MiB files: the files behind
    the first two wait >= 14 ms each in the queue, so the planner gives them
    prefixes above its floor; RF_SHA_NO_PREFIX plans the same set without.
    WAIT takes them all, RACE whichever it finds; digests equal the oracle."""
    c = capi.Context(0, host_threads=1)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    rng = np.random.default_rng(8)
    lens = np.concatenate([[24 * MiB + 64 * i + i for i in range(8)],
                           rng.integers(1, 64 * 1024, size=500)]).astype(np.uint64)
    ds = GenSet(c, lens, 0xABC)
    want = _want_stream(oracle, lens, 0xABC)
    plan = c.sha_plan(ds.offs, ds.lens, 0)
    st = plan.prefix_stats()
    print("planner: %d host files, %d prefixed, %.1f MiB planned" % (plan.stats().n_host, st.n_prefixed,
                                                                    st.planned_bytes / MiB))
    assert 0 < st.n_prefixed <= plan.stats().n_host - 2
    for _ in range(2):
        assert (ds.run(c, plan) == want).all()
        r = plan.prefix_stats()
        print("race: taken %d missed %d" % (r.taken, r.missed))
        assert r.taken + r.missed == st.n_prefixed
    plan.set_prefixes(None, capi.RF_PREFIX_WAIT)
    assert (ds.run(c, plan) == want).all()
    r = plan.prefix_stats()
    assert r.taken == st.n_prefixed and r.missed == 0 and r.skipped_bytes == st.planned_bytes
    plan.close()
    plan = c.sha_plan(ds.offs, ds.lens, capi.RF_SHA_NO_PREFIX)
    assert plan.prefix_stats().n_prefixed == 0
    assert (ds.run(c, plan) == want).all()
    plan.close()
    ds.free()
    c.close()


def test_only_all_host_runs_calibrate_the_link(oracle):
    """rf_host_link stays the built-in estimate after a hybrid run whose host
    leg took > 1 GiB and after a host-resident batch; an RF_SHA_ALL_HOST run
    of the same set measures it."""
    c = capi.Context(0)
    if c.host_info()[0] == 0:
        pytest.skip("host leg unavailable (no SHA extensions)")
    assert c.host_link()[1] is False
    lens = np.array([288 * MiB] * 4 + [4096] * 2000, dtype=np.uint64)
    ds = GenSet(c, lens, 31)
    plan = c.sha_plan(ds.offs, ds.lens, 0)
    assert plan.stats().host_bytes >= 1 << 30
    ds.run(c, plan)
    plan.close()
    assert c.host_link()[1] is False
    msgs = [oracle.fill_stream(i, 3 * MiB) for i in range(4)]
    assert c.sha256_batch(msgs) == [oracle.sha256(m) for m in msgs]
    assert c.host_link()[1] is False
    plan = c.sha_plan(ds.offs, ds.lens, capi.RF_SHA_ALL_HOST)
    ds.run(c, plan)
    plan.close()
    rate, measured = c.host_link()
    assert measured and rate > 0
    ds.free()
    c.close()
