"""GPU parity of K2's byte-2 fast path (cb0 = 2: split block 0, the producer's
operand hand-off, the block-1 pre-build, sf_pos, hash_fused_chain_lean) on
ragged graphs, in every level form.

The graphs (k2_shapes.ragged; their mix is asserted in test_k2_shapes.py)
keep every fusion target's hole at material byte 2, so the loader keeps
fuse_pos2, and make the lanes of one wave disagree: next targets of 1, 2 and
3+ blocks up to 12, chains of depth 0..7 ending in a sink, in a multi-hole
job or beside a queued twin, heads with and without a midstate, levels 1 to
257 queueable jobs wide.  Each test loads a graph under one form's knobs
(read at load), sets every input, recomputes in full and steps through change
sets of 1, 63, 64, 65, 96, 97 and all input slots, every other slot re-set to
the value it has (cut-off: its chain is not rehashed).  After every step the
whole slot table equals the oracle's (OGraph.update replaying the slots that
really changed; orc_graph_check re-deriving every job from the table's own
holes), recompute's count equals the oracle's (the exact dirty closure), and
rf_graph_stats says the form under test ran."""
import numpy as np
import pytest

import k2_shapes as K
import reflow_oracle as O

pytestmark = pytest.mark.gpu

STEPS = (1, 63, 64, 65, 96, 97, None)  # None: every input slot
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    from reflow_amd import capi
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


_REF = {}


def reference(name):
    """The oracle's run of graph `name`, computed once and left unchanged:
    (inputs, full table, [(slots, values, table, jobs hashed)] per step)."""
    if name not in _REF:
        a, info = K.graph(name)
        n_in = info["n_in"]
        rng = np.random.default_rng(len(name) + info["n_jobs"])
        inputs = rng.integers(0, 256, size=(n_in, 32), dtype=np.uint8)
        og = O.OGraph(a)
        og.set_inputs(np.arange(n_in), inputs)
        og.full()
        full = og.slots[:a["n_slots"]].copy()
        steps = []
        for k in STEPS:
            pick = rng.choice(n_in, size=n_in if k is None else k, replace=False).astype(np.uint32)
            values = og.slots[pick].copy()  # every other slot keeps its value
            values[::2] = rng.integers(0, 256, size=(len(pick[::2]), 32), dtype=np.uint8)
            hashed = og.update(pick[::2], values[::2])
            steps.append((pick, values, og.slots[:a["n_slots"]].copy(), hashed))
        og.close()
        for v in (inputs, full, *(x for st in steps for x in st[:3])):
            v.setflags(write=False)
        _REF[name] = (inputs, full, steps)
    return _REF[name]


def load(ctx, monkeypatch, name, **env):
    """Graph `name` loaded under the given knobs, inputs set, recomputed in full."""
    from reflow_amd import capi
    a, info = K.graph(name)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    g = capi.Graph.from_arrays(ctx, a)
    for k in env:
        monkeypatch.delenv(k)
    inputs, full, _ = reference(name)
    g.set_slots(np.arange(info["n_in"], dtype=np.uint32), inputs)
    g.recompute(full=True)
    check(g, name, full, "full")
    return g


def check(g, name, want, where, n=None, hashed=None):
    a, info = K.graph(name)
    table = g.get_slots(np.arange(a["n_slots"], dtype=np.uint32))
    bad = np.nonzero((table != want).any(axis=1))[0]
    if len(bad):  # the lane shape of the first wrong job, from the generator's record
        j = int(bad[0]) - info["n_in"]
        what = (info["role"][j], int(info["level"][j]), int(info["blocks"][j]), int(info["holes"][j])) \
            if "role" in info and j >= 0 else None
        raise AssertionError((name, where, len(bad), "first wrong job, (role, level, blocks, holes)", j, what))
    assert O.check_slots(a, table, 8) == (0, None), (name, where)
    if hashed is not None:
        assert n == hashed, (name, where, n, hashed)
    return table


def step(g, name, i):
    """Step i of the reference run on g; returns the count of the change set."""
    pick, values, table, hashed = reference(name)[2][i]
    g.set_slots(pick, values)
    mark_lf = g.stats().last_mark_lf
    n = g.recompute(full=False)
    check(g, name, table, ("step", i, len(pick)), n, hashed)
    return len(pick), mark_lf


def latency_stats(g, where):
    st = g.stats()
    assert (st.last_levels_lf, st.last_levels_half) == (0, 0), where


@pytest.mark.parametrize("name", ["sf2", "sf8", "sf40", "mix"])
def test_latency_form_split_modes(ctx, monkeypatch, name):
    """k2_level_pl<2>, the default: block 0 split in mode 2, in mode 1, and
    cb0 = 2 without a split -- each against the oracle, so all three tables
    are equal slot for slot."""
    gs = [load(ctx, monkeypatch, name), load(ctx, monkeypatch, name, RF_K2_SPLIT=1),
          load(ctx, monkeypatch, name, RF_K2_SPLIT=0)]
    assert [g.stats().split_block0 for g in gs] == [2, 1, 0]  # (fuse_pos2 held: the loader kept the split)
    for i in range(len(STEPS)):
        for g in gs:
            _, mark_lf = step(g, name, i)
            assert mark_lf == 0
            latency_stats(g, (name, i))
            assert g.stats().last_levels_oct == 0
    for g in gs:
        g.close()


@pytest.mark.parametrize("name", ["sf8", "mix"])
def test_wide_form(ctx, monkeypatch, name):
    """k2_level_pl<3> (every level counted as one of long jobs)."""
    g = load(ctx, monkeypatch, name, RF_K2_WIDE=1)
    assert g.stats().split_block0 == 2
    for i in range(len(STEPS)):
        step(g, name, i)
        latency_stats(g, (name, i))
    g.close()


@pytest.mark.parametrize("split_half", [0, 1])
@pytest.mark.parametrize("name", ["sf8", "sf40"])
def test_half_workgroups(ctx, monkeypatch, name, split_half):
    """k2_level_pl<2, false, 32> on a pretended 1-CU chip: every launched
    level has at least 97 jobs (test_k2_shapes.test_level_forms), so each runs
    in half workgroups when 65 or 96 slots were marked and none does for 64
    or 97; with and without block 0 split in them.  The same graph loaded
    wide runs only its top level so (queueable jobs nobody reads: no chains
    to average, a level of short jobs whatever RF_K2_WIDE says) -- that the
    ragged levels run k2_level_pl<3> there is read from this."""
    g = load(ctx, monkeypatch, name, RF_K2_OVF_CU=1, RF_K2_SPLIT_HALF=split_half)
    gw = load(ctx, monkeypatch, name, RF_K2_OVF_CU=1, RF_K2_WIDE=1)
    assert g.stats().split_block0 == 2
    n_form = sum(1 for w in K.analyze(K.graph(name)[0])["width"] if w)
    assert n_form == len(K.GRAPHS[name]["widths"]) + 1
    for i in range(len(STEPS)):
        k, _ = step(g, name, i)
        assert g.stats().last_levels_half == (n_form if k in (65, 96) else 0), (name, k)
        assert g.stats().last_levels_lf == 0
        step(gw, name, i)
        assert gw.stats().last_levels_half == (1 if k in (65, 96) else 0), (name, k)
    g.close()
    gw.close()


@pytest.mark.parametrize("name", ["sf2", "sf40", "mix"])
def test_throughput_form(ctx, monkeypatch, name):
    """k2_level_lf and k3_mark_slots_lf at every width."""
    g = load(ctx, monkeypatch, name, RF_K2_THRU=0)
    assert g.stats().split_block0 == 2
    n_form = sum(1 for w in K.analyze(K.graph(name)[0])["width"] if w)
    for i in range(len(STEPS)):
        _, mark_lf = step(g, name, i)
        assert mark_lf == 1
        assert g.stats().last_levels_lf == n_form, (name, i)
    g.close()


def test_forms_switched_per_step(ctx, monkeypatch):
    """Under the default thresholds, latency and throughput steps in turn
    (rf_graph_set_forms): each form reads the dirty bits, lists and counters
    the other left."""
    from reflow_amd import capi
    name = "sf8"
    g = load(ctx, monkeypatch, name)
    for i in range(len(STEPS)):
        thru = i % 2 == 1
        if thru:
            g.set_forms(0)
        else:
            g.set_forms(capi.Graph.THRU_DEFAULT, capi.Graph.THRU_WIDE_DEFAULT, capi.Graph.THRU_MARK_DEFAULT)
        _, mark_lf = step(g, name, i)
        assert mark_lf == (1 if thru else 0)
        assert (g.stats().last_levels_lf >= 1) == thru, (i, g.stats().last_levels_lf)
    g.close()


@pytest.mark.parametrize("name", ["merge2", "merge40"])
def test_octo_form(ctx, monkeypatch, name):
    """k2_level_oct on a level of few long multi-hole jobs above the ragged
    byte-2 levels, against the same graph with the octo form off."""
    g, gp = load(ctx, monkeypatch, name), load(ctx, monkeypatch, name, RF_K2_OCT=0)
    assert g.stats().split_block0 == 2
    for i in range(len(STEPS)):
        step(g, name, i)
        step(gp, name, i)
        assert g.stats().last_levels_oct >= 1 and gp.stats().last_levels_oct == 0
    g.close()
    gp.close()


@pytest.mark.parametrize("launch", ["latency", "throughput", "octo"])
@pytest.mark.parametrize("n_sinks", [127, 128, 129])
def test_attached_sink_list(ctx, monkeypatch, n_sinks, launch):
    """127, 128 and 129 sinks in the sink level, its list attached to a
    latency-form launch (sink lanes), a throughput-form one or the octo
    form's, wherever RF_K2_SINK_AT puts it."""
    name = ("msink" if launch == "octo" else "sink") + str(n_sinks)
    an = K.analyze(K.graph(name)[0])
    assert (an["level"] == an["sink_level"]).sum() == n_sinks
    env = {"RF_K2_THRU": 0} if launch == "throughput" else {}
    for sink_at in range(5):
        g = load(ctx, monkeypatch, name, RF_K2_SINK_AT=sink_at, **env)
        assert g.stats().split_block0 == 2
        for i in range(len(STEPS)):
            step(g, name, i)
            st = g.stats()
            assert st.last_sink_attach != NONE and st.last_sink_attach < an["sink_level"], (sink_at, i)
            if launch == "throughput":
                assert st.last_levels_lf >= 1
            elif sink_at == 0:  # the fill level's launch
                assert st.last_sink_attach == an["fill_level"]
            if launch == "octo":
                assert st.last_levels_oct >= 1
                if sink_at == 0:
                    assert an["fill_level"] == K.graph(name)[1]["cap_level"]  # the octo level's own launch
            else:
                assert st.last_levels_oct == 0
        g.close()


@pytest.mark.parametrize("name", ["sf8", "mix"])
def test_checkpoint_keeps_split(ctx, monkeypatch, tmp_path, name):
    from reflow_amd import capi
    g = load(ctx, monkeypatch, name)
    for i in range(3):
        step(g, name, i)
    path = str(tmp_path / "shapes.ckpt")
    g.save(path)
    r = capi.Graph.restore(ctx, path)
    assert r.stats().split_block0 == g.stats().split_block0 == 2
    for i in range(3, len(STEPS)):
        step(g, name, i)
        step(r, name, i)
        latency_stats(r, (name, i))
    g.close()
    r.close()


def test_negative_control_hole_at_byte_3(ctx, monkeypatch):
    """One fusion target's hole at byte 3: no byte-2 fast path, the general
    path takes over and the tables still match."""
    g = load(ctx, monkeypatch, "break")
    assert g.stats().split_block0 == 0
    for i in range(len(STEPS)):
        step(g, "break", i)
    g.close()


def test_throughput_form_grid_stride(ctx, monkeypatch):
    """k2_level_lf's grid is capped at 1024 workgroups of 256 lanes: a level
    of 262,144 + 257 listed heads takes a second grid-stride iteration."""
    from reflow_amd import capi
    a, info = K.graph("stride")
    n_in = info["n_in"]
    assert info["widths"][0] > 1024 * 256
    rng = np.random.default_rng(7)
    every = np.arange(a["n_slots"], dtype=np.uint32)
    monkeypatch.setenv("RF_K2_THRU", "0")
    g = capi.Graph.from_arrays(ctx, a)
    monkeypatch.delenv("RF_K2_THRU")
    assert g.stats().split_block0 == 2
    g.set_slots(np.arange(n_in, dtype=np.uint32), rng.integers(0, 256, size=(n_in, 32), dtype=np.uint8))
    g.recompute(full=True)
    # every input changes, so every job is in the dirty closure and the
    # oracle's table is its full evaluation of the new inputs
    inputs = rng.integers(0, 256, size=(n_in, 32), dtype=np.uint8)
    g.set_slots(np.arange(n_in, dtype=np.uint32), inputs)
    assert g.stats().last_mark_lf == 1
    n = g.recompute(full=False)
    assert g.stats().last_levels_lf >= 1
    assert n == info["n_jobs"]
    og = O.OGraph(a)
    og.set_inputs(np.arange(n_in), inputs)
    og.full()
    table = g.get_slots(every)
    assert (table == og.slots[:a["n_slots"]]).all()
    assert O.check_slots(a, table, 8) == (0, None)
    og.close()
    g.close()
