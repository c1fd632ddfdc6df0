"""The ragged byte-2 graphs (k2_shapes) really hold the mix the GPU tests
(test_gpu_dag_shapes.py) rely on -- asserted on the arrays alone, through
k2_shapes.analyze's restatement of the loader's level and fusion rule: every
single-hole reader of a job output at byte 2, the requested level widths,
every 64-job slice of the loader's order mixed in its lanes' next-target
block counts, chain depths and midstates, every padding-edge length present.
And the oracle's graph evaluation against hashlib on one of them, so the
GPU tests' reference does not rest on the project's own SHA-256 alone."""
import hashlib

import numpy as np
import pytest

import k2_shapes as K
import reflow_oracle as O

NAMES = list(K.GRAPHS) + ["stride"]


@pytest.fixture(scope="module", params=NAMES)
def built(request):
    a, info = K.graph(request.param)
    return request.param, a, info, K.analyze(a)


def test_block_count_edges():
    assert [K.nblocks(n) for n in (55, 56, 119, 120, 183, 184, 247, 248)] == [1, 2, 2, 3, 3, 4, 4, 5]
    assert sorted(K._BY_BLOCKS) == [1, 2, 3] and sum(map(len, K._BY_BLOCKS.values())) == len(K.EDGE_LENGTHS)


def test_every_width_is_used():
    seen = set()
    for name in K.GRAPHS:
        seen.update(K.GRAPHS[name]["widths"])
    assert seen >= set(K.WIDTHS)


def test_every_slot_fused_setting_is_used():
    assert {K.GRAPHS[name]["sf"] for name in K.GRAPHS} == set(K.SF_SETTINGS)


def test_chain_tails(built):
    """Every way a chain ends occurs: in a sink, in a hole of a multi-hole
    job, and beside a queued twin (a single-hole reader of a job output that
    is not the fused one); twins head chains of their own."""
    name, a, info, an = built
    if name == "stride":
        return
    tails = an["fused_target"] & (an["fuse"] < 0)
    assert (tails & an["sink"]).any() and (tails & ~an["sink"]).any()
    twins = an["queueable"] & (an["holes"] == 1)
    assert twins.sum() >= 1
    if len(info["widths"]) >= 3:  # (a twin sits one level above its producer, below the cap level: two-level
        # graphs hold a handful, all at level 1)
        assert twins.sum() >= 8 and (an["depth"][twins] > 0).any() and (an["depth"][twins] == 0).any()
    # a twin's producer has a fusion target of its own, at the twin's level
    slot = np.asarray(a["hole_slot"], np.int64)[np.asarray(a["hole_ptr"][:-1], np.int64)[twins]]
    prod = an["producer"][slot]
    assert (prod >= 0).all() and (an["fuse"][prod] >= 0).all()
    assert (an["level"][an["fuse"][prod]] == an["level"][twins]).all()
    assert sorted(set(info["tail"].values())) == ["open", "twin"]


def test_byte2_property(built):
    name, a, info, an = built
    n_in = info["n_in"]
    single = an["holes"] == 1
    reads_job = np.zeros(len(single), bool)
    reads_job[single] = np.asarray(a["hole_slot"])[np.asarray(a["hole_ptr"][:-1], np.int64)[single]] >= n_in
    bad = single & reads_job & ((an["first_pos"] != 2) | (an["lead"] != 0))
    if name == "break":
        assert np.nonzero(bad)[0].tolist() == [info["broken"]]
        assert an["fused_target"][info["broken"]]  # a fusion target: the loader must clear fuse_pos2
    else:
        assert not bad.any(), np.nonzero(bad)[0][:10]
    assert an["fused_target"].sum() > 0
    # slot-fused jobs: at one position without leading blocks (sf_pos), or mixed
    sfp = set(an["first_pos"][an["slot_fused"]].tolist())
    if info["sf"] == "mix":
        assert sfp == {2, 8, 40}
    elif info["sf"] is not None:
        assert sfp == {info["sf"]} and not an["lead"][an["slot_fused"]].any()


def test_level_widths(built):
    name, a, info, an = built
    want = info["widths"]
    assert an["width"][:len(want)].tolist() == list(want)
    if name == "stride":
        return
    assert an["width"][info["cap_level"]] == info["cap_width"]
    # the generator's record agrees with the loader's rule
    assert (an["level"][an["sink_level"] != an["level"]] == info["level"][an["sink_level"] != an["level"]]).all()
    roles = np.array(info["role"])
    assert (an["fused_target"] == (roles == "chain")).all()
    assert (an["slot_fused"] == (roles == "sf")).all()
    assert (an["depth"][info["heads"]] == info["depth"][info["heads"]]).all()
    assert (an["blocks"] == info["blocks"]).all() and (an["holes"] == info["holes"]).all()
    n_sinks = K.GRAPHS[name].get("sinks", 0)
    if n_sinks:
        moved = an["level"] == an["sink_level"]
        assert moved.sum() == n_sinks and (roles[moved] == "sink").all()
        assert an["fill_level"] == (info["cap_level"] if K.GRAPHS[name].get("merge") else len(want) - 1)
    else:
        assert an["sink_level"] is None
    if K.GRAPHS[name].get("merge"):  # the octo form's level: few long jobs, no fusion target among them
        at = an["level"] == info["cap_level"]
        assert (an["fuse"][at] < 0).all() and an["blocks"][at].max() <= 32 and an["holes"][at].max() <= 64
        assert an["blocks"][at].mean() >= 8 and (an["queueable"][at]).all()


def test_level_forms(built):
    """What the form choice reads (capi.cpp, k2_graph.hip graph_level_half):
    the ragged levels average under 8 blocks a queueable job, so they are
    levels of short jobs by default; and on the graphs the half-workgroup test
    uses no launched level has 65..96 jobs, so that min(level jobs, marked
    slots) is in (64, 96] exactly for change sets of 65..96 slots."""
    name, a, info, an = built
    q = an["queueable"] & ~an["sink"]
    for l in range(len(info["widths"])):
        at = q & (an["level"] == l)
        assert at.any() and (info["widths"][l] == 1 or an["blocks"][at].mean() < 8), (name, l)
    if name in ("sf8", "sf40"):
        launched = an["jobs_at"][an["width"] > 0]
        assert (launched >= 97).all(), launched


def test_mixed_slices(built):
    name, a, info, an = built
    order = an["order"]
    order = order[an["queueable"][order]]
    lv = an["level"][order]
    n_slices = 0
    for l in np.nonzero(an["width"] >= 64)[0]:
        if l == an["sink_level"] or (name != "stride" and l >= len(info["widths"])):
            continue
        jobs = order[lv == l]
        for s in range(0, len(jobs) - 63, 64):
            sl = jobs[s:s + 64]
            nxt = np.where(an["fuse"][sl] >= 0, an["blocks"][np.maximum(an["fuse"][sl], 0)], 0)
            where = (name, int(l), s)
            assert len(set(nxt[nxt > 0].tolist())) >= 3, where
            halves = [set(np.minimum(h[h > 0], 3).tolist()) for h in (nxt[:32], nxt[32:])]
            assert {1, 2, 3} in halves, where  # a 1-, a 2- and a 3+-block target in one 32-job half
            depths = set(an["depth"][sl].tolist())
            assert len(depths) >= 3 and 0 in depths, where
            mid = an["lead"][sl] > 0
            assert mid.any() and not mid.all(), where
            n_slices += 1
    assert n_slices >= 1


def test_length_coverage(built):
    name, a, info, an = built
    lens = np.asarray(a["tmpl_len"])[an["fused_target"]]
    have = set(lens.tolist())
    assert have >= set(K.EDGE_LENGTHS), sorted(set(K.EDGE_LENGTHS) - have)
    assert set(an["blocks"][an["fused_target"]].tolist()) & set(K.LONG_BLOCKS)
    assert int(an["depth"].max()) >= 7


def test_oracle_graph_matches_hashlib():
    a, info = K.graph("mix")
    n_in = info["n_in"]
    rng = np.random.default_rng(5)
    inputs = rng.integers(0, 256, size=(n_in, 32), dtype=np.uint8)
    og = O.OGraph(a)
    og.set_inputs(np.arange(n_in), inputs)
    og.full()
    val = [bytes(r) for r in inputs] + [None] * info["n_jobs"]
    blob = bytes(a["blob"])
    ptr, pos, slot = (np.asarray(a[k]).tolist() for k in ("hole_ptr", "hole_pos", "hole_slot"))
    for j, (o, off, n) in enumerate(zip(a["out_slot"].tolist(), a["tmpl_off"].tolist(), a["tmpl_len"].tolist())):
        m = bytearray(blob[off:off + n])
        for h in range(ptr[j], ptr[j + 1]):
            m[pos[h]:pos[h] + 32] = val[slot[h]]
        val[o] = hashlib.sha256(m).digest()
    assert og.slots[:a["n_slots"]].tobytes() == b"".join(val)
    # and an incremental step: the oracle's table after update == hashlib's from scratch
    assert O.check_slots(a, og.slots, 1) == (0, None)
    og.close()
