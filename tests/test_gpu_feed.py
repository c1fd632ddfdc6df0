"""GPU parity of the graph change feed (rf_graph_feed_*, k6_feed.hip).

The expected result is always derived on the CPU: the oracle's OGraph (full,
then update) gives the slot table after every step, and a model of the feed
keeps what was delivered so far -- a poll must report exactly the tracked
job-output slots whose oracle rows differ from what was last delivered (or
from the table at open), ascending, with the oracle's rows.  Listed polls
(the candidates of one plain step) are also checked against forced-scan polls
on a twin graph, byte for byte."""
import hashlib

import numpy as np
import pytest

import reflow_oracle as O
from reflow_amd.workloads import Dag1000
from test_gpu_dag_fusion import load as load_jobs
from test_gpu_dag_fusion import random_jobs
from test_gpu_dag_oct import wide_jobs

pytestmark = pytest.mark.gpu

PHYS = ("pR1", "pE1", "pE2", "pE3", "pES", "pXS")


@pytest.fixture(scope="module")
def ctx():
    from reflow_amd import capi
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def h32(rows, tag):
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 32)
    return np.frombuffer(b"".join(hashlib.sha256(r.tobytes() + tag).digest() for r in rows),
                         dtype=np.uint8).reshape(-1, 32).copy()


def jobs_arrays(n_in, jobs):
    """rf_graph_desc arrays of (out slot, template, [(pos, slot)]) jobs."""
    blob, off, ln, hp, hpos, hslot = bytearray(), [], [], [0], [], []
    for out, tmpl, holes in jobs:
        off.append(len(blob))
        ln.append(len(tmpl))
        blob += tmpl
        for p, s in holes:
            hpos.append(p)
            hslot.append(s)
        hp.append(len(hpos))
    return dict(n_slots=n_in + len(jobs), out_slot=np.array([o for o, _, _ in jobs], np.uint32),
                tmpl_off=np.array(off, np.uint64), tmpl_len=np.array(ln, np.uint32), hole_ptr=np.array(hp, np.uint64),
                hole_pos=np.array(hpos, np.uint32), hole_slot=np.array(hslot, np.uint32), blob=bytes(blob))


def flat_arrays(n_slots, holes):
    """J = n_slots // 2 jobs over the input slots [0, n_slots - J): job j
    reads input j (one hole: slot-fused, hashed by the mark kernel) or inputs
    j and j + 1 (two holes: listed), and writes slot n_slots - J + j -- so the
    job outputs end at the table's last slot."""
    J = n_slots // 2
    n_in = n_slots - J
    j = np.arange(J, dtype=np.uint32)
    tlen = 2 + 34 * holes + 6
    stride = (tlen + 15) // 16 * 16
    blob = np.zeros((J, stride), dtype=np.uint8)
    for h in range(holes):
        blob[:, 34 * h:34 * h + 2] = (0, 5)
    blob[:, 34 * holes:34 * holes + 4] = j[:, None] >> np.array([0, 8, 16, 24]) & 255
    hole_slot = np.stack([(j + h) % n_in for h in range(holes)], axis=1).reshape(-1)
    hole_pos = np.tile(np.array([34 * h + 2 for h in range(holes)], np.uint32), J)
    return dict(n_slots=n_slots, out_slot=(n_in + j).astype(np.uint32), tmpl_off=(j.astype(np.uint64) * stride),
                tmpl_len=np.full(J, tlen, np.uint32), hole_ptr=np.arange(J + 1, dtype=np.uint64) * holes,
                hole_pos=hole_pos.astype(np.uint32), hole_slot=hole_slot.astype(np.uint32), blob=blob.tobytes()), n_in


class Tracked:
    """A GPU graph with a feed, its oracle twin and the model of what the
    feed has delivered."""

    def __init__(self, ctx, a, in_slots, in_digests, forms=None, mask=None, open_feed=True):
        from reflow_amd import capi
        self.ctx, self.a = ctx, a
        self.g = capi.Graph.from_arrays(ctx, a)
        if forms is not None:
            self.g.set_forms(*forms)
        self.g.set_slots(in_slots, in_digests)
        self.g.recompute(full=True)
        self.o = O.OGraph(a)
        self.o.set_inputs(in_slots, in_digests)
        self.o.full()
        self.tracked = np.zeros(int(a["n_slots"]), dtype=bool)
        self.tracked[np.asarray(a["out_slot"], dtype=np.int64)] = True
        if mask is not None:
            self.tracked &= mask
        self.reported = self.o.slots[:int(a["n_slots"])].copy()
        if open_feed:
            self.g.feed_open(mask)

    def cpu_update(self, slots, digests):
        self.o.update(slots, digests)

    def gpu_step(self, slots, digests, how="host"):
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        digests = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        if how == "host":
            self.g.set_slots(slots, digests)
            self.g.recompute(full=False)
        else:  # mark + step in one asynchronous call
            ds, dd = self.ctx.upload(slots), self.ctx.upload(digests)
            self.g.update_recompute_async(ds.ptr, dd.ptr, len(slots))
            self.ctx.sync()

    def step(self, slots, digests, how="host"):
        self.cpu_update(slots, digests)
        self.gpu_step(slots, digests, how)

    def expect(self):
        now = self.o.slots[:len(self.reported)]
        s = np.nonzero(self.tracked & (now != self.reported).any(axis=1))[0].astype(np.uint32)
        return s, now[s].copy()

    def deliver(self, slots, digests):
        self.reported[slots] = digests

    def poll_check(self, cap=None, flags=0, mode=None):
        """One poll against the model; returns the expected (slots, digests)."""
        es, ed = self.expect()
        s, d, found = self.g.feed_poll(cap=cap, flags=flags)
        n = len(es) if cap is None else min(len(es), cap)
        assert found == len(es), (found, len(es))
        assert s.tolist() == es[:n].tolist()
        assert (d == ed[:n]).all()
        if mode is not None:
            assert self.g.feed_stats().last_mode == mode
        self.deliver(es[:n], ed[:n])
        return es, ed

    def close(self):
        self.g.close()
        self.o.close()


def dag_steps(dag):
    """One file, 1 % of the files, every file, back to the old IDs."""
    slots, old, new = dag.change_set(0.01)
    return [(slots[:1], new[:1]), (slots, new), (dag.file_slots, h32(dag.leaf_ids, b"v3")),
            (dag.file_slots, dag.leaf_ids)]


# ---- 1. the feed against the oracle ------------------------------------------
@pytest.mark.parametrize("how", ["host", "update_async"])
@pytest.mark.parametrize("forms", [None, (0, 0, 0)], ids=["default_forms", "throughput_forms"])
def test_feed_against_oracle(ctx, forms, how):
    from reflow_amd import capi
    dag = Dag1000(22, 32)
    t = Tracked(ctx, dag.arrays(), dag.file_slots, dag.leaf_ids, forms=forms)
    assert t.g.feed_stats().tracked_slots == dag.n_jobs
    es, _ = t.poll_check(mode=capi.RF_FEED_LISTED)
    assert len(es) == 0
    for slots, digs in dag_steps(dag):
        t.step(slots, digs, how)
        es, _ = t.poll_check(mode=capi.RF_FEED_LISTED)
        assert len(es) > 0
        assert t.g.feed_poll()[2] == 0  # an immediate second poll
        assert t.g.feed_stats().last_mode == capi.RF_FEED_LISTED
    if forms is not None:
        st = t.g.stats()
        assert st.last_levels_lf >= 1 and st.last_mark_lf == 1
    # the digests the slots already hold: cut off at the mark
    slots, _, _ = dag.change_set(0.01)
    t.step(slots, dag.leaf_ids[slots], how)
    es, _ = t.poll_check(mode=capi.RF_FEED_LISTED)
    assert len(es) == 0
    t.close()


# ---- 2. listed == scan ----------------------------------------------------------
def case_dag(S):
    dag = Dag1000(S, 32)
    return dag.arrays(), dag.file_slots, dag.leaf_ids, dag_steps(dag)


def case_jobs(n_in, jobs, picks, seed):
    rng = np.random.default_rng(seed)
    inputs = rng.integers(0, 256, size=(n_in, 32), dtype=np.uint8)
    steps = []
    for k in picks:
        pick = np.sort(rng.choice(n_in, size=k, replace=False)).astype(np.uint32)
        digs = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        digs[1::2] = inputs[pick[1::2]]  # every other change re-sets the same value
        inputs[pick] = digs
        steps.append((pick, digs.copy()))
    return jobs_arrays(n_in, jobs), np.arange(n_in, dtype=np.uint32), inputs_at_start(n_in, seed), steps


def inputs_at_start(n_in, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n_in, 32), dtype=np.uint8)


CASES = {
    "dag22": lambda: case_dag(22),
    "dag400": lambda: case_dag(400),
    "random21": lambda: case_jobs(64, random_jobs(21, 64), [6, 6, 6, 6], 21),
    "random22": lambda: case_jobs(64, random_jobs(22, 64), [6, 6, 6, 6], 22),
    "random23": lambda: case_jobs(64, random_jobs(23, 64), [6, 6, 6, 6], 23),
    "wide": lambda: case_jobs(600, wide_jobs(3, 600), [1, 7, 60, 600, 3], 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_listed_equals_scan(ctx, name):
    from reflow_amd import capi
    a, in_slots, in_digs, steps = CASES[name]()
    tl = Tracked(ctx, a, in_slots, in_digs)
    ts = Tracked(ctx, a, in_slots, in_digs)
    total = 0
    for slots, digs in steps:
        for t in (tl, ts):
            t.step(slots, digs)
        sl, dl, fl = tl.g.feed_poll()
        ss, dsc, fs = ts.g.feed_poll(flags=capi.RF_FEED_FORCE_SCAN)
        assert tl.g.feed_stats().last_mode == capi.RF_FEED_LISTED
        assert ts.g.feed_stats().last_mode == capi.RF_FEED_SCAN
        assert fl == fs and sl.tobytes() == ss.tobytes() and dl.tobytes() == dsc.tobytes()
        es, ed = tl.expect()
        assert sl.tolist() == es.tolist() and (dl == ed).all()
        tl.deliver(es, ed)
        total += fl
    assert total > 0
    st = tl.g.feed_stats()
    assert st.polls == st.polls_listed == len(steps) and ts.g.feed_stats().polls_scan == len(steps)
    if name == "wide":
        assert tl.g.stats().last_levels_oct >= 1
    tl.close()
    ts.close()


def test_listed_with_jobs_loaded_through_the_fusion_loader(ctx):
    """The raw-job loader of test_gpu_dag_fusion gives the graph jobs_arrays
    describes: the feed's first listed poll on it equals the oracle's."""
    from reflow_amd import capi
    n_in, jobs = 64, random_jobs(24, 64)
    a = jobs_arrays(n_in, jobs)
    ins = inputs_at_start(n_in, 24)
    t = Tracked(ctx, a, np.arange(n_in, dtype=np.uint32), ins, open_feed=False)
    t.g.close()
    t.g = load_jobs(ctx, n_in, jobs)
    t.g.set_slots(np.arange(n_in, dtype=np.uint32), ins)
    t.g.recompute(full=True)
    t.g.feed_open()
    t.step(np.array([3, 40], np.uint32), h32(ins[[3, 40]], b"x"))
    es, _ = t.poll_check(mode=capi.RF_FEED_LISTED)
    assert len(es) > 0
    t.close()


# ---- 3. fallbacks ------------------------------------------------------------------
def test_two_steps_before_one_poll_scan(ctx):
    from reflow_amd import capi
    dag = Dag1000(22, 32)
    t = Tracked(ctx, dag.arrays(), dag.file_slots, dag.leaf_ids)
    slots, old, new = dag.change_set(0.02)
    half = len(slots) // 2
    other, _, other_new = dag.change_set(0.01, seed=99)
    t.step(slots, new)
    before = t.expect()[0]
    # the first half back to the old IDs (changed and reverted: absent), others changed
    t.step(np.concatenate([slots[:half], other]), np.concatenate([old[:half], other_new]))
    es, _ = t.poll_check(mode=capi.RF_FEED_SCAN)
    assert 0 < len(es) and len(set(before.tolist()) - set(es.tolist())) > 0
    assert t.g.feed_poll()[2] == 0
    # and the feed is listed again after it
    t.step(slots[:half], new[:half])
    assert len(t.poll_check(mode=capi.RF_FEED_LISTED)[0]) > 0
    t.close()


def test_full_recompute_and_unstepped_marks_scan(ctx):
    from reflow_amd import capi
    dag = Dag1000(22, 32)
    t = Tracked(ctx, dag.arrays(), dag.file_slots, dag.leaf_ids)
    slots, old, new = dag.change_set(0.01)
    t.cpu_update(slots, new)
    t.g.set_slots(slots, new)
    t.g.recompute(full=True)
    assert len(t.poll_check(mode=capi.RF_FEED_SCAN)[0]) > 0
    # slots set after the step: the mark kernels already hashed their slot-fused chains
    t.step(slots, old)
    other, _, other_new = dag.change_set(0.01, seed=7)
    t.g.set_slots(other, other_new)
    s, d, found = t.g.feed_poll()
    assert t.g.feed_stats().last_mode == capi.RF_FEED_SCAN and found > 0
    t.g.recompute(full=False)
    s2, d2, _ = t.g.feed_poll()
    # both polls together: the table now against the table at the last checked poll
    t.cpu_update(other, other_new)
    es, ed = t.expect()
    got = dict(zip(s.tolist(), d.tolist()))
    got.update(zip(s2.tolist(), d2.tolist()))
    assert sorted(got) == es.tolist() and all(got[x] == ed[i].tolist() for i, x in enumerate(es.tolist()))
    t.close()


def test_open_preconditions(ctx):
    from reflow_amd import capi
    dag = Dag1000(2, 3)
    a = dag.arrays()
    g = capi.Graph.from_arrays(ctx, a)
    g.set_slots(dag.file_slots, dag.leaf_ids)

    def refused(fn, code=capi.RF_EPRECONDITION):
        with pytest.raises(capi.RfError) as e:
            fn()
        assert e.value.code == code, e.value

    refused(g.feed_open)  # never recomputed
    refused(g.feed_poll)  # no feed
    g.recompute(full=True)
    slots, old, new = dag.change_set(0.5)
    g.set_slots(slots, new)
    refused(g.feed_open)  # a change set is pending
    g.recompute(full=False)
    g.feed_open()
    refused(g.feed_open)  # a second open
    none = np.zeros(0, np.uint32)
    refused(lambda: g.set_part(dict(nranks=1, rank=0, max_export=0, export_slot=none, import_slot=none,
                                    import_bid=none, any_import=False)))
    g.feed_close()
    refused(g.feed_close)
    g.feed_open()  # and it opens again
    assert g.feed_poll()[2] == 0
    g.close()  # (frees the feed)


# ---- 4. cap ------------------------------------------------------------------------
def test_cap_slices_and_a_step_between_partial_polls(ctx):
    from reflow_amd import capi
    dag = Dag1000(22, 32)
    t = Tracked(ctx, dag.arrays(), dag.file_slots, dag.leaf_ids)
    slots, old, new = dag.change_set(0.01)
    t.step(slots, new)
    n = len(t.expect()[0])
    assert n >= 100
    s, d, found = t.g.feed_poll(cap=0)  # a count
    assert (found, len(s)) == (n, 0) and t.g.feed_stats().last_mode == capi.RF_FEED_LISTED
    seen = []
    for _ in range(3):
        es, _ = t.poll_check(cap=7)
        seen += es[:7].tolist()
    # a step between two partial polls: some delivered slots move again, some pending ones move back
    other, _, other_new = dag.change_set(0.01, seed=5)
    t.step(np.concatenate([slots[:len(slots) // 2], other]), np.concatenate([old[:len(slots) // 2], other_new]))
    polls = 0
    while True:
        es, _ = t.poll_check(cap=7, mode=capi.RF_FEED_LISTED)
        polls += 1
        if len(es) == 0:
            break
        assert es[:7].tolist() == sorted(set(es[:7].tolist()))
    assert polls > 3 and seen == sorted(set(seen))
    t.close()


# ---- 5. mask ------------------------------------------------------------------------
def test_mask_of_physical_keys(ctx):
    from reflow_amd import capi
    dag = Dag1000(22, 32)
    a = dag.arrays()
    mask = np.zeros(dag.n_slots, dtype=bool)
    for k in PHYS:
        mask[dag.kinds[k].out_slot] = True
    t = Tracked(ctx, a, dag.file_slots, dag.leaf_ids, mask=mask)
    assert t.g.feed_stats().tracked_slots == int(mask.sum())
    everything = Tracked(ctx, a, dag.file_slots, dag.leaf_ids)
    for slots, digs in dag_steps(dag)[1:]:
        t.step(slots, digs)
        everything.step(slots, digs)
        es, _ = t.poll_check(mode=capi.RF_FEED_LISTED)
        all_s, _ = everything.poll_check(mode=capi.RF_FEED_LISTED)
        assert len(es) > 0 and es.tolist() == [s for s in all_s.tolist() if mask[s]]
    t.close()
    everything.close()


def test_mask_bits_refused(ctx):
    from reflow_amd import capi
    a, n_in = flat_arrays(1000, 1)  # 1000 % 64 != 0: the last mask word has bits past n_slots
    ins = inputs_at_start(n_in, 1)
    t = Tracked(ctx, a, np.arange(n_in, dtype=np.uint32), ins, open_feed=False)
    for bad in (0, n_in - 1, 1000, 1023):  # input slots; at and beyond n_slots
        words = np.zeros(16, dtype=np.uint64)
        words[(n_in + 5) // 64] |= np.uint64(1) << np.uint64((n_in + 5) % 64)  # (a job output: fine)
        words[bad // 64] |= np.uint64(1) << np.uint64(bad % 64)
        with pytest.raises(capi.RfError) as e:
            t.g.feed_open(words)
        assert e.value.code == capi.RF_EINVAL, (bad, e.value)
    words = np.zeros(16, dtype=np.uint64)
    words[(n_in + 5) // 64] |= np.uint64(1) << np.uint64((n_in + 5) % 64)
    t.g.feed_open(words)
    assert t.g.feed_stats().tracked_slots == 1
    t.close()


# ---- 6. bitmap and tile edges ---------------------------------------------------------
@pytest.mark.parametrize("holes", [1, 2], ids=["slot_fused", "listed"])
@pytest.mark.parametrize("d", [-1, 0, 1, 63, 64, 65])
@pytest.mark.parametrize("k", [1, 2])
def test_tile_edges(ctx, k, d, holes):
    from reflow_amd import capi
    n_slots = k * capi.FEED_TILE_SLOTS + d
    a, n_in = flat_arrays(n_slots, holes)
    J = n_slots // 2
    rng = np.random.default_rng(1000 * k + 10 * (d + 1) + holes)
    ins = rng.integers(0, 256, size=(n_in, 32), dtype=np.uint8)
    t = Tracked(ctx, a, np.arange(n_in, dtype=np.uint32), ins)
    assert t.g.feed_stats().tracked_slots == J
    # the inputs whose change moves: no job, the first job's output, the
    # last job's (the table's last slot), every job's, every 64th job's
    sets = [np.zeros(0, np.uint32), np.array([0], np.uint32), np.array([J - 1], np.uint32),
            np.arange(J, dtype=np.uint32), np.arange(0, J, 64, dtype=np.uint32)]
    for i, pick in enumerate(sets):
        if len(pick):
            t.step(pick, rng.integers(0, 256, size=(len(pick), 32), dtype=np.uint8))
        else:
            t.g.recompute(full=False)  # a step with nothing marked
        es, _ = t.poll_check(mode=capi.RF_FEED_LISTED)
        # (input 0 is also job J - 1's second hole when there are exactly J inputs)
        want = {0: 0, 1: holes if n_in == J else 1, 2: holes, 3: J}.get(i)
        if want is not None:
            assert len(es) == want, (i, len(es))
        if i == 2:
            assert es[-1] == n_slots - 1
        assert t.g.feed_poll()[2] == 0
    # and a forced scan finds the same after one more change
    t.step(sets[4], rng.integers(0, 256, size=(len(sets[4]), 32), dtype=np.uint8))
    t.poll_check(flags=capi.RF_FEED_FORCE_SCAN, mode=capi.RF_FEED_SCAN)
    t.close()


# ---- 7. fused lookup --------------------------------------------------------------------
def test_fused_lookup(ctx):
    from reflow_amd import capi
    dag = Dag1000(22, 32)
    a = dag.arrays()
    t1 = Tracked(ctx, a, dag.file_slots, dag.leaf_ids)
    t2 = Tracked(ctx, a, dag.file_slots, dag.leaf_ids)
    slots, old, new = dag.change_set(0.01)
    rng = np.random.default_rng(4)
    assoc = capi.Assoc(ctx, 4096)
    KIND = 3

    def lookup(t, live, cap):
        d_slots, d_keys, d_vals = ctx.alloc(4 * cap), ctx.alloc(32 * cap), ctx.alloc(32 * cap)
        d_status, d_n2 = ctx.alloc(cap), ctx.alloc(16)
        d_status.fill(0xEE)
        d_vals.fill(0xEE)
        t.g.feed_lookup_device(live, assoc, KIND, cap, d_slots.ptr, d_keys.ptr, d_status.ptr, d_vals.ptr, d_n2.ptr)
        ctx.sync()
        found, written = d_n2.to_numpy(np.uint64).tolist()
        status, vals = d_status.to_numpy(np.uint8), d_vals.to_numpy(np.uint8).reshape(-1, 32)
        assert (status[written:] == 0xEE).all() and (vals[written:] == 0xEE).all()  # rows not written: untouched
        return (found, d_slots.to_numpy(np.uint32)[:written], d_keys.to_numpy(np.uint8).reshape(-1, 32)[:written],
                status[:written], vals[:written])

    def composed(t, live, cap):
        s, d, found = t.g.feed_poll(cap=cap)
        vals, fnd = assoc.get(KIND, d)
        status = fnd.copy()
        if live is not None:
            out = live.probe(d) == 0
            status[out] = 2
            vals[out] = 0
        return found, s, d, status, vals

    def cpu(keys, live_words, table):
        status = np.zeros(len(keys), np.uint8)
        vals = np.zeros((len(keys), 32), np.uint8)
        hit = np.ones(len(keys), np.uint8)
        if live_words is not None:
            m, kk, length, words = live_words
            O.lib().orc_bloomlive_contains_batch(words.ctypes.data, length, m, kk, keys.tobytes(), len(keys),
                                                 hit.ctypes.data, 1)
        for i, key in enumerate(keys):
            if not hit[i]:
                status[i] = 2
            elif key.tobytes() in table:
                status[i], vals[i] = 1, np.frombuffer(table[key.tobytes()], np.uint8)
        return status, vals

    for step, (digs, use_live, cap) in enumerate([(new, True, 4096), (old, False, 4096), (new, True, 50)]):
        for t in (t1, t2):
            t.step(slots, digs)
        es, ed = t1.expect()
        assert len(es) >= 100
        # values for every second expected key, three quarters of the keys in the liveset
        table = {ed[i].tobytes(): rng.integers(1, 256, size=32, dtype=np.uint8).tobytes() for i in range(0, len(es), 2)}
        st = assoc.put(KIND, np.frombuffer(b"".join(table), np.uint8), np.frombuffer(b"".join(table.values()), np.uint8))
        assert (st == 0).all()
        live = live_words = None
        if use_live:
            m, kk = O.estimate_parameters(len(es), 0.01)
            live = capi.Bloom.new(ctx, m, kk)
            live.add(ed[np.arange(len(es)) % 4 != 3])
            live_words = (m, kk, live.params()[2], live.words())
        off = 0
        while True:  # (cap below found: the rest arrive with the next call)
            f1, s1, k1, st1, v1 = lookup(t1, live, cap)
            f2, s2, k2, st2, v2 = composed(t2, live, cap)
            assert f1 == f2 == len(es) - off
            n = min(f1, cap)
            assert s1.tolist() == s2.tolist() == es[off:off + n].tolist()
            assert (k1 == k2).all() and (k1 == ed[off:off + n]).all()
            assert (st1 == st2).all() and (v1 == v2).all()
            cs, cv = cpu(ed[off:off + n], live_words, table)
            assert (st1 == cs).all() and (v1 == cv).all()
            if use_live:
                assert set(st1.tolist()) == {0, 1, 2} or n < 8
            else:
                assert set(st1.tolist()) == {0, 1}
            off += n
            if f1 <= cap:
                break
        assert off == len(es)
        assert (step == 2) == (cap < len(es))
        t1.deliver(es, ed)
        if live is not None:
            live.close()
    t1.close()
    t2.close()
