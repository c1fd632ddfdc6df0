"""The evaluation waves on the device (rf_eval_wave_*, k10_wave.hip) against
their CPU model (tests/wave_model.py: Eval.todo + Eval.lookup in bottom-up
mode and the completion step, eval.go:902-955, 1163-1269): after begin and
after every step and reject, the states of every node, each of the five lists
in both scopes byte for byte, the hits' which / values / masks and the
counts -- for the reference's three bottom-up flows, seeded random flows
(tests/wave_cases.py), hand-built shapes at the kernels' edges, absent keys,
refusals, keys read from a loaded graph, the hand-over from a top-down plan,
and runs repeated on another stream, over a table that grew and was compacted
and with the finished set split differently."""
import numpy as np
import pytest

import plan_model as P
import reflow_oracle as O
import wave_cases as C
import wave_model as W
from reflow_amd import capi

pytestmark = pytest.mark.gpu

KIND = C.KIND


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


# ---- helpers ---------------------------------------------------------------------
def results(w):
    """Everything a wave object reports, as bytes."""
    s = w.stats()
    out = {"states": w.states().tobytes(), "counts": list(s.counts),
           "stats": (s.mode, s.waves, s.last_wave, s.looked_up, s.keys_probed, s.keys_filtered)}
    for scope in (W.ALL, W.LAST):
        for state in range(5):
            out[scope, state] = tuple(a.tobytes() for a in w.list(state, scope))
    return out


def compare(w, m):
    assert w.states().tolist() == m.states.tolist()
    s = w.stats()
    assert list(s.counts) == m.counts()
    assert (s.mode, s.waves, s.last_wave) == (m.mode, m.waves, len(m.last))
    assert (s.looked_up, s.keys_probed, s.keys_filtered) == (m.looked_up, m.keys_probed, m.keys_filtered)
    assert s.n_nodes == m.n and s.rounds <= s.depth
    for scope in (W.ALL, W.LAST):
        for state in range(5):
            nodes, which, vals, mask = w.list(state, scope)
            wn, ww, wv, wm = m.list(state, scope)
            assert nodes.dtype == np.uint32 and nodes.tobytes() == wn.tobytes(), (scope, state)
            if state == W.HIT:
                assert which.tobytes() == ww.tobytes() and mask.tobytes() == wm.tobytes(), scope
                assert vals.tobytes() == wv.tobytes(), scope


def flat_keys(node_keys):
    return P.key_arrays(node_keys)[1]


class Both(C.ModelTarget):
    """A scenario's calls on the device object and on the model; check() compares."""

    def __init__(self, ctx, case, capacity=1024):
        super().__init__(case)
        self.dev = capi.Assoc(ctx, capacity)
        self.dlive = None if self.live is None else capi.Bloom.load(ctx, self.live.m, self.live.k, self.live.words,
                                                                    self.live.length)
        dep_ptr, deps = P.flow_csr(case.nodes)
        key_ptr, _ = P.key_arrays(case.keys())
        self.w = capi.EvalWave(ctx, dep_ptr, deps, self.model.flags, key_ptr)

    def put(self, kind, keys, vals):
        super().put(kind, keys, vals)
        if keys:
            st = self.dev.put(kind, np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(vals), np.uint8))
            assert (st == capi.RF_OK).all()

    def begin(self, roots, keys, no_cache_extern=False):
        super().begin(roots, keys, no_cache_extern)
        self.w.begin(roots, self.dev, KIND, keys=flat_keys(keys), live=self.dlive, no_cache_extern=no_cache_extern)

    def step(self, finished, keys):
        super().step(finished, keys)
        self.w.step(finished, self.dev, KIND, keys=flat_keys(keys), live=self.dlive)

    def reject(self, nodes):
        super().reject(nodes)
        self.w.reject(nodes)

    def check(self):
        compare(self.w, self.model)

    def close(self):
        self.w.close()
        self.dev.close()
        if self.dlive is not None:
            self.dlive.close()


class Hand:
    """A hand-built graph (dep index lists, flag bytes, per-node key lists) on
    the device and in the model, over one pair of tables."""

    def __init__(self, ctx, dep_lists, flags, node_keys, cached=(), second_only=()):
        self.keys = node_keys
        self.ref = O.InmemoryAssoc()
        self.dev = capi.Assoc(ctx, 1024)
        ks, vs = [], []
        for i in cached:
            for k in (node_keys[i][-1:] if i in second_only else node_keys[i]):
                if k != W.ZERO:
                    ks.append(k)
                    vs.append(P.fileset_id(i))
        self.put(ks, vs)
        ptr = np.zeros(len(dep_lists) + 1, np.uint64)
        ptr[1:] = np.cumsum([len(d) for d in dep_lists])
        deps = np.array([x for d in dep_lists for x in d], np.uint32)
        self.m = W.Wave(dep_lists=dep_lists, flags=flags)
        key_ptr, self.flat = P.key_arrays(node_keys)
        self.w = capi.EvalWave(ctx, ptr, deps, np.array(flags, np.uint8), key_ptr)

    def put(self, keys, vals):
        if keys:
            st = self.dev.put(KIND, np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(vals), np.uint8))
            assert (st == capi.RF_OK).all()
            for k, v in zip(keys, vals):
                self.ref.put(KIND, None, k, v)

    def begin(self, roots, nce=False):
        self.m.begin(roots, self.ref, KIND, self.keys, no_cache_extern=nce)
        self.w.begin(roots, self.dev, KIND, keys=self.flat, no_cache_extern=nce)
        compare(self.w, self.m)

    def step(self, finished):
        self.m.step(finished, self.ref, KIND, self.keys)
        self.w.step(finished, self.dev, KIND, keys=self.flat)
        compare(self.w, self.m)

    def reject(self, nodes):
        self.m.reject(nodes)
        self.w.reject(nodes)
        compare(self.w, self.m)

    def open_nodes(self):
        return [int(i) for i in list(self.m.list(W.READY)[0]) + list(self.m.list(W.HIT)[0])]

    def to_the_end(self):
        """Everything READY or HIT finishes, step after step.  Returns the waves' sizes."""
        sizes = []
        while self.open_nodes():
            self.step(self.open_nodes())
            sizes.append(len(self.m.last))
        assert self.m.counts()[W.TODO] == 0
        return sizes

    def close(self):
        self.w.close()
        self.dev.close()


def hand_keys(flags, two=()):
    two = set(two)
    return [([C.fake_key(b"phys", i)] if i in two else []) + [C.fake_key(b"logical", i)] if f & W.F_CACHEABLE else []
            for i, f in enumerate(flags)]


# ---- 1. the reference's behavioural flows ---------------------------------------------
def _executed(nodes, ran):
    return {i for i in ran if P.flow_flags([nodes[i]])[0] & P.F_CACHEABLE}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cache_lookup_bottomup_flow(ctx, seed):
    """TestCacheLookupBottomup (test/evaltest/eval_test.go:232-277): exec(a) is
    a hit, exec(b) and the extern run; completions are split across steps by
    the seed and the finished nodes' keys are Put between steps."""
    nodes, ix = W.cache_lookup_bottomup_flow()
    case = C.FlowCase(nodes, [ix["extern"]], [ix["intern"], ix["exec_a"]], seed)
    t = Both(ctx, case)
    seen = C.play(case, t, accept=lambda i: True, foreign=0.0, write=1.0)
    assert _executed(nodes, seen["ran"]) == {ix["extern"], ix["exec_b"]}
    assert set(seen["accepted"]) == {ix["intern"], ix["exec_a"]} and seen["which"] == {0, 1}
    assert t.model.states.tolist().count(W.DONE) == len(nodes)
    # evaluated again, the entries written meanwhile serve every cacheable node: later waves hit
    for f in nodes:
        f.done = f.op == O.OP["OpVal"]
    seen = C.play(case, t, accept=lambda i: True, foreign=0.0, write=1.0)
    assert _executed(nodes, seen["ran"]) == set() and seen["late_hits"] >= 1 and ix["extern"] in seen["accepted"]
    t.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_cache_lookup_missing_flow(ctx, seed):
    """TestCacheLookupMissing (:279-312): the exec's hit fails the caller's
    missing() check, is rejected and runs."""
    nodes, ix = W.cache_lookup_missing_flow()
    case = C.FlowCase(nodes, [ix["exec"]], [ix["intern"], ix["exec"]], seed)
    t = Both(ctx, case)
    seen = C.play(case, t, accept=lambda i: i != ix["exec"], foreign=0.0, write=1.0)
    assert _executed(nodes, seen["ran"]) == {ix["exec"]} and seen["rejected"] == 1
    t.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_no_cache_extern_flow(ctx, seed):
    """TestNoCacheExtern (:314-351), bottom-up: the extern is cached and a root
    -- it runs all the same, and so do both execs."""
    nodes, ix = W.cache_lookup_bottomup_flow()
    case = C.FlowCase(nodes, [ix["extern"]], [ix["intern"], ix["extern"]], seed)
    t = Both(ctx, case)
    seen = C.play(case, t, accept=lambda i: True, no_cache_extern=True, foreign=1.0, write=1.0)
    assert _executed(nodes, seen["ran"]) == {ix["exec_a"], ix["exec_b"], ix["extern"]}
    t.close()
    # the consumer of an extern is looked up bottom-up (Eval.lookup never calls dirty)
    nodes, ix = P.no_cache_extern_flow()
    case = C.FlowCase(nodes, [ix["top"], ix["clean_root"]], range(len(nodes)), seed)
    t = Both(ctx, case)
    seen = C.play(case, t, accept=lambda i: True, no_cache_extern=True, foreign=0.0, write=0.0)
    assert ix["consumer"] in seen["accepted"] and ix["clean"] in seen["accepted"]
    assert {ix["extern"], ix["top"], ix["clean_root"]} <= set(seen["ran"])
    t.close()


# ---- 2. random flows ------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,with_liveset", C.SEEDS)
def test_random_flows(ctx, seed, n, with_liveset):
    """What these cover is asserted on the model alone by tests/test_wave_model.py."""
    case = C.Case(seed, n, with_liveset)
    t = Both(ctx, case)
    seen = C.play(case, t)
    assert seen["states"] == {0, 1, 2, 3, 4} and (seen["filtered"] > 0) == with_liveset
    assert all(t.model.states[r] == W.DONE for r in case.roots)
    t.close()


# ---- 3. shape edges -------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 200])
def test_consumer_of_k_deps(ctx, k):
    """Node 0 lists k leaves (and, for k >= 63, one of them twice): ready when
    all have finished -- in one step, and again one dep per step, only at the last."""
    dl = list(range(1, k + 1))
    if k >= 63:
        dl.append(dl[k // 2])
    dep_lists = [dl] + [[] for _ in range(k)]
    flags = [W.F_CACHEABLE] * (k + 1)
    keys = hand_keys(flags, two=[0])
    h = Hand(ctx, dep_lists, flags, keys, cached=[0] + list(range(1, k + 1, 3)), second_only=[0])
    h.begin([0])
    assert h.m.pending[0] == len(dl) and len(h.m.last) == k and h.w.stats().rounds >= 1
    h.step(list(range(1, k + 1)))
    assert sorted(h.m.last) == [0] and h.m.hits[0][0] == 1
    h.begin([0, 0])
    for i, d in enumerate(np.random.default_rng(k).permutation(k) + 1):
        h.step([int(d)])
        assert (sorted(h.m.last) == [0]) == (i == k - 1)
    h.close()


@pytest.mark.parametrize("k", [63, 64, 65, 130])
def test_finished_node_with_k_consumers(ctx, k):
    """Leaf k has k consumers 0..k-1 (one lists it three times, one also waits on
    another leaf); a second finished node rides in the same wavefront."""
    dep_lists = [[k] for _ in range(k)] + [[], []]
    dep_lists[1] = [k, k, k]
    dep_lists[2] = [k, k + 1]
    flags = [W.F_CACHEABLE if i % 2 else 0 for i in range(k + 2)]
    keys = hand_keys(flags)
    h = Hand(ctx, dep_lists, flags, keys, cached=range(1, k, 4))
    h.begin(list(range(k)))
    assert sorted(h.m.last) == [k, k + 1]
    h.step([k, k])  # listed twice: one decrement per consumer entry
    assert sorted(h.m.last) == [i for i in range(k) if i != 2] and h.m.pending[2] == 1
    h.step([k + 1])
    assert sorted(h.m.last) == [2]
    h.begin(list(range(k)))
    h.step([k + 1, k])  # both in one step
    assert len(h.m.last) == k
    h.close()


def test_unreached_consumers_stay_unseen(ctx):
    """Nodes 3 and 4 list reached nodes but are beneath no root: never decremented, never in a wave."""
    dep_lists = [[1], [2], [], [1, 2], [2, 3]]
    flags = [W.F_CACHEABLE] * 5
    h = Hand(ctx, dep_lists, flags, hand_keys(flags), cached=[3, 4])
    h.begin([0])
    assert h.m.states.tolist() == [W.TODO, W.TODO, W.READY, W.UNSEEN, W.UNSEEN]
    sizes = h.to_the_end()
    assert sizes == [1, 1, 0] and h.m.states.tolist() == [W.DONE] * 3 + [W.UNSEEN] * 2
    h.close()


@pytest.mark.parametrize("width", [63, 64, 65, 255, 256, 257])
def test_wave_widths(ctx, width):
    """A wave of `width` nodes, each over its own leaf, under one root of degree `width`."""
    dep_lists = [list(range(1, width + 1))] + [[width + i] for i in range(1, width + 1)] + [[] for _ in range(width)]
    n = 2 * width + 1
    flags = [W.F_CACHEABLE if i % 3 else 0 for i in range(n)]
    keys = hand_keys(flags, two=range(0, n, 2))  # i % 4: 0 cached under its second key only, 2 under both, 3 not
    h = Hand(ctx, dep_lists, flags, keys, cached=[i for i in range(1, n) if i % 4 != 3], second_only=range(0, n, 4))
    h.begin([0])
    assert len(h.m.last) == width
    h.step(list(range(width + 1, n)))
    assert len(h.m.last) == width and W.HIT in h.m.states[1:width + 1] and W.READY in h.m.states[1:width + 1]
    assert {h.m.hits[i][0] for i in range(1, width + 1) if h.m.states[i] == W.HIT} == {0, 1}
    h.step(list(range(1, width + 1)))
    assert sorted(h.m.last) == [0]
    h.close()


def test_wave_wider_than_a_launch(ctx):
    """Wave 0 and the wave after it are wider than the resolve kernel's grid has lanes: the grid strides."""
    probe = capi.EvalWave(ctx, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint8),
                          np.zeros(2, np.uint64))
    lanes = 1024 * 256  # the largest grid: read back below
    width = lanes + 1000
    probe.close()
    n = 2 * width + 1
    ptr = np.zeros(n + 1, np.uint64)
    ptr[1] = width
    ptr[2:width + 2] = width + np.arange(1, width + 1)
    ptr[width + 2:] = 2 * width
    deps = np.concatenate([np.arange(1, width + 1), np.arange(width + 1, n)]).astype(np.uint32)
    flags = np.zeros(n, np.uint8)
    cacheable = np.arange(1, width + 1, 997)
    flags[cacheable] = W.F_CACHEABLE
    key_ptr = np.zeros(n + 1, np.uint64)
    key_ptr[1:] = np.cumsum(flags == W.F_CACHEABLE)
    keys = [C.fake_key(b"logical", int(i)) for i in cacheable]
    assoc = capi.Assoc(ctx, 1024)
    hit = cacheable[::2]
    assoc.put(KIND, np.frombuffer(b"".join(keys[::2]), np.uint8),
              np.frombuffer(b"".join(P.fileset_id(int(i)) for i in hit), np.uint8))
    w = capi.EvalWave(ctx, ptr, deps, flags, key_ptr)
    flat = np.frombuffer(b"".join(keys), np.uint8)
    w.begin([0], assoc, KIND, keys=flat)
    s = w.stats()
    assert s.wave_lanes == lanes and s.last_wave == width and list(s.counts) == [0, width + 1, width, 0, 0]
    assert w.list(W.READY, W.LAST)[0].tolist() == list(range(width + 1, n))
    w.step(np.arange(width + 1, n), assoc, KIND, keys=flat)
    s = w.stats()
    assert s.last_wave == width and s.looked_up == len(cacheable) and s.counts[W.HIT] == len(hit)
    nodes, which, vals, mask = w.list(W.HIT, W.LAST)
    assert nodes.tolist() == hit.tolist() and (which == 0).all() and (mask == 1).all()
    assert vals.tobytes() == b"".join(P.fileset_id(int(i)) for i in hit)
    ready = w.list(W.READY)[0]
    assert len(ready) == width - len(hit) and w.states()[0] == W.TODO
    w.step(np.concatenate([nodes, ready]), assoc, KIND, keys=flat)
    assert w.list(W.READY, W.LAST)[0].tolist() == [0]
    w.close()
    assoc.close()


@pytest.mark.parametrize("n", [1, 2, 3, 33, 70])
def test_small_and_odd_sizes(ctx, n):
    """n = 1, and n no multiple of 4 or 32: a chain with a shortcut."""
    dep_lists = [([i + 1] + ([n - 1] if i + 2 < n else [])) if i + 1 < n else [] for i in range(n)]
    flags = [W.F_CACHEABLE] * n
    h = Hand(ctx, dep_lists, flags, hand_keys(flags), cached=range(0, n, 2))
    h.begin([0])
    assert h.to_the_end()[-1] == 0 and h.m.counts()[W.DONE] == n
    h.close()


def test_chain_of_depth_40(ctx):
    """One node per wave; the descent takes more than three batches of rounds."""
    n = 40
    dep_lists = [[i + 1] for i in range(n - 1)] + [[]]
    flags = [W.F_CACHEABLE] * n
    h = Hand(ctx, dep_lists, flags, hand_keys(flags), cached=range(0, n, 3))
    h.begin([0])
    s = h.w.stats()
    assert s.depth == n and n <= s.rounds <= s.depth and s.round_batch * 3 < n and s.last_wave == 1
    assert h.to_the_end() == [1] * (n - 1) + [0]
    assert [x[0] for x in h.m.history[:-1]] == list(range(n - 1, -1, -1))
    h.close()


def test_roots_twice_done_root_no_roots_empty_steps(ctx):
    dep_lists = [[2, 3], [3, 4], [5], [5], [], []]
    flags = [W.F_CACHEABLE, 0, W.F_CACHEABLE, W.F_CACHEABLE, W.F_CACHEABLE, W.F_CACHEABLE]
    h = Hand(ctx, dep_lists, flags, hand_keys(flags), cached=[3, 5])
    h.begin([0, 1, 0, 1, 1])  # roots given twice
    assert h.m.states.tolist() == [W.TODO, W.TODO, W.TODO, W.TODO, W.READY, W.HIT]
    h.step([])  # n == 0: an empty wave, nothing else changes
    assert not h.m.last and h.m.waves == 2 and h.m.states.tolist().count(W.TODO) == 4
    h.step([5])
    assert sorted(h.m.last) == [2, 3] and h.m.states[3] == W.HIT
    h.to_the_end()
    # a done root is DONE and not expanded; a done dep satisfies its consumer from the start
    for i in (1, 5):
        flags[i] |= W.F_DONE
    h.m.set_flags([1, 5], [flags[1], flags[5]])
    h.w.set_flags([1, 5, 5], [flags[1], 0, flags[5]])  # listed twice: the last value holds
    h.begin([1, 0])
    assert h.m.states.tolist() == [W.TODO, W.DONE, W.READY, W.HIT, W.UNSEEN, W.DONE] and sorted(h.m.last) == [2, 3]
    h.to_the_end()
    # no roots: nothing is reached
    h.begin([])
    assert h.m.states.tolist() == [W.UNSEEN] * 6 and h.w.stats().rounds == 0 and not h.m.last
    h.step([])
    h.close()
    # no nodes at all
    empty = capi.EvalWave(ctx, np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8),
                          np.zeros(0, np.uint64))
    assoc = capi.Assoc(ctx, 64)
    empty.begin([], assoc, KIND)
    empty.step([], assoc, KIND)
    assert empty.stats().depth == 0 and list(empty.stats().counts) == [0] * 5 and empty.stats().waves == 2
    assert all(len(empty.list(s, sc)[0]) == 0 for s in range(5) for sc in (W.ALL, W.LAST)) and len(empty.states()) == 0
    empty.begin_states(np.zeros(0, np.uint8))
    empty.close()
    assoc.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_list_tile_edges_and_caps(ctx, delta):
    """tile - 1 / tile / tile + 1 nodes in a state, in both scopes; the cap rule."""
    probe = capi.EvalWave(ctx, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint8),
                          np.zeros(2, np.uint64))
    tile = probe.stats().list_tile
    probe.close()
    k = tile + delta  # leaves 1..k under root 0, and 7 more leaves under root k + 1
    dep_lists = [list(range(1, k + 1))] + [[] for _ in range(k)] + [list(range(k + 2, k + 9))] + [[] for _ in range(7)]
    n = len(dep_lists)
    flags = [W.F_CACHEABLE] * n
    keys = hand_keys(flags)
    h = Hand(ctx, dep_lists, flags, keys, cached=range(k + 2, n))
    h.begin([0, k + 1])
    assert h.m.counts()[W.READY] == k and h.m.counts()[W.HIT] == 7  # k nodes READY: the tile edge, scope ALL and LAST
    h.step(list(range(k + 2, n)))
    assert h.m.counts()[W.READY] == k + 1 and h.m.counts()[W.DONE] == 7 and sorted(h.m.last) == [k + 1]
    h.step(list(range(1, k + 1)))
    assert h.m.counts()[W.DONE] == k + 7  # k + 7 DONE nodes across the tiles; the last wave is node 0 alone
    h.begin([0, k + 1])
    for state, scope in ((W.READY, W.ALL), (W.READY, W.LAST), (W.HIT, W.LAST)):
        full = h.w.list(state, scope)
        found = len(full[0])
        assert found == (7 if state == W.HIT else k) and h.w.count(state, scope) == found
        carried = 4 if state == W.HIT else 1
        exact = h.w.list(state, scope, cap=found, poison=0xAB)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(exact[:carried], full[:carried]))
        with pytest.raises(capi.RfError) as e:
            h.w.list(state, scope, cap=found - 1, poison=0xAB)
        assert e.value.code == capi.RF_EINVAL and e.value.needed == found
        nodes_b, which_b, vals_b, kf_b = e.value.buffers
        assert nodes_b[found - 1:].tobytes() == b"\xab" * 4 * len(nodes_b[found - 1:])
        for buf in (which_b, vals_b, kf_b):
            assert (buf[found - 1:] == 0xAB).all()
    # the device form: ranks below cap are written, the count is whole
    cap = 3
    d_nodes, d_which, d_vals = capi.DeviceBuffer(ctx, 4 * 16), capi.DeviceBuffer(ctx, 16), capi.DeviceBuffer(ctx, 32 * 16)
    d_kf, d_n = capi.DeviceBuffer(ctx, 16), capi.DeviceBuffer(ctx, 8)
    for b in (d_nodes, d_which, d_vals, d_kf):
        b.fill(0xAB)
    h.w.list_device(W.HIT, W.LAST, cap, d_nodes.ptr, d_which.ptr, d_vals.ptr, d_kf.ptr, d_n.ptr)
    ctx.sync()
    wn, ww, wv, wm = h.m.list(W.HIT, W.LAST)
    assert d_n.to_numpy(np.uint64)[0] == len(wn) == 7
    assert d_nodes.to_numpy(np.uint32)[:cap].tobytes() == wn[:cap].tobytes()
    assert (d_nodes.to_numpy(np.uint32)[cap:] == 0xABABABAB).all()
    assert d_which.to_numpy()[:cap].tobytes() == ww[:cap].tobytes() and (d_which.to_numpy()[cap:] == 0xAB).all()
    assert d_kf.to_numpy()[:cap].tobytes() == wm[:cap].tobytes() and (d_kf.to_numpy()[cap:] == 0xAB).all()
    assert d_vals.to_numpy()[:32 * cap].tobytes() == wv[:cap].tobytes() and (d_vals.to_numpy()[32 * cap:] == 0xAB).all()
    for b in (d_nodes, d_which, d_vals, d_kf, d_n):
        b.free()
    h.close()


# ---- 4. absent keys, refusals -----------------------------------------------------------
def test_absent_keys(ctx):
    """Rows [zeros, logical]: which == 1, mask 0b10, one key probed; all rows absent: not looked up."""
    flags = [W.F_CACHEABLE] * 4
    keys = [[W.ZERO, C.fake_key(b"logical", 0)], [W.ZERO, W.ZERO], [C.fake_key(b"phys", 2), W.ZERO],
            [W.ZERO, C.fake_key(b"logical", 3)]]
    h = Hand(ctx, [[], [], [], []], flags, keys, cached=[0, 1, 2])
    h.begin([0])
    assert h.m.hits[0] == (1, P.fileset_id(0), 0b10)
    s = h.w.stats()
    assert (s.looked_up, s.keys_probed, s.keys_filtered) == (1, 1, 0)
    which, mask = h.w.list(W.HIT)[1:4:2]
    assert which.tolist() == [1] and mask.tolist() == [0b10]
    h.begin([0, 1, 2, 3])
    assert h.m.states.tolist() == [W.HIT, W.READY, W.HIT, W.READY]
    s = h.w.stats()
    assert (s.looked_up, s.keys_probed) == (3, 3) and h.m.hits[2][0] == 0
    h.close()


def test_refusals_leave_every_result_unchanged(ctx):
    dep_lists = [[1, 2, 2], [3], [3], [], []]
    flags = [W.F_CACHEABLE] * 5
    h = Hand(ctx, dep_lists, flags, hand_keys(flags), cached=[3])
    with pytest.raises(capi.RfError) as e:  # before any begin
        h.w.step([3], h.dev, KIND, keys=h.flat)
    assert e.value.code == capi.RF_EPRECONDITION
    h.begin([0])
    before = results(h.w)

    def refused(call, code=capi.RF_EINVAL):
        with pytest.raises(capi.RfError) as e:
            call()
        assert e.value.code == code and results(h.w) == before
        compare(h.w, h.m)
    refused(lambda: h.w.step([3, 1], h.dev, KIND, keys=h.flat))          # a TODO node
    refused(lambda: h.w.step([3, 4], h.dev, KIND, keys=h.flat))          # an UNSEEN node
    refused(lambda: h.w.step([5], h.dev, KIND, keys=h.flat))             # out of range
    refused(lambda: h.w.reject([3, 0]))                                  # a TODO node
    refused(lambda: h.w.begin_states([W.TODO, W.UNSEEN, W.DONE, W.DONE, 0]))  # an UNSEEN dep under a TODO
    refused(lambda: h.w.begin_states([W.DONE, W.DONE, W.DONE, W.DONE, 5]))    # no such state
    refused(lambda: h.w.begin([7], h.dev, KIND, keys=h.flat))            # a root out of range
    h.step([3])
    before = results(h.w)
    refused(lambda: h.w.reject([1]))                                     # READY, not a hit
    refused(lambda: h.w.step([3], h.dev, KIND, keys=h.flat))             # DONE already
    # objects of two contexts
    other = capi.Context(0, host_threads=0)
    foreign = capi.Assoc(other, 64)
    refused(lambda: h.w.step([1], foreign, KIND, keys=h.flat))
    refused(lambda: h.w.begin([0], foreign, KIND, keys=h.flat))
    live = capi.Bloom.load(other, 64, 1, np.zeros(1, np.uint64), 64)
    refused(lambda: h.w.step([1], h.dev, KIND, keys=h.flat, live=live))
    live.close()
    foreign.close()
    other.close()
    h.step([1, 2])
    assert sorted(h.m.last) == [0]
    h.close()


# ---- 5. keys from a graph ---------------------------------------------------------------
def test_keys_from_a_graph(ctx):
    """An exec over an exec: the assoc holds the parent's physical key for one
    particular child value only.  After the child finishes: set_slots,
    recompute, step -- the parent is a HIT under key 0; with another value it
    is READY.  The child's value is one file whose ID is an input slot of the graph."""
    from lowering import Lowerer
    unset = bytes(32)
    val = O.OFlow("OpVal", value=W.files("in"), done=True)
    child = O.OFlow("OpExec", [val], image="img", cmd="child", done=True,
                    value=O.OFileset(map={"out": (unset, 3)}))  # (done while lowering: the parent gets a physical job)
    parent = O.OFlow("OpExec", [child], image="img", cmd="parent")
    nodes = [parent, child, val]
    low = Lowerer(file_slots=True)
    key_ptr, key_slots = [0], []
    for f in nodes:
        ps = low.lower_physical(f)
        if ps is not None:
            key_slots.append(ps)
        key_slots.append(low.lower(f))
        key_ptr.append(len(key_slots))
    assert key_ptr == [0, 2, 4, 5]
    key_slots = np.array(key_slots, np.uint32)
    value_slot = low.L.file_slot[unset]
    child.done = False
    g = capi.Graph.from_arrays(ctx, low.L.arrays())
    files = list(low.L.file_slot.items())
    dep_ptr, deps = P.flow_csr(nodes)
    flags = P.flow_flags(nodes)
    assert flags.tolist() == [W.F_CACHEABLE, W.F_CACHEABLE, W.F_DONE]
    w = capi.EvalWave(ctx, dep_ptr, deps, flags, np.array(key_ptr, np.uint64), key_slots)
    m = W.Wave(nodes)
    ref, dev = O.InmemoryAssoc(), capi.Assoc(ctx, 64)
    with pytest.raises(capi.RfError) as e:  # never recomputed
        w.begin([0], dev, KIND, graph=g)
    assert e.value.code == capi.RF_EPRECONDITION

    def node_keys():
        rows = g.get_slots(key_slots)
        return [[rows[r].tobytes() for r in range(key_ptr[i], key_ptr[i + 1])] for i in range(len(nodes))]
    # the entry was computed from the child value `good`
    good, other = O.sha256(b"the child's output"), O.sha256(b"another output")
    child.value.map["out"] = (good, 3)
    child.done = True
    wanted = parent.physical_digest()
    child.done = False
    fs_parent = P.fileset_id(0)
    ref.put(KIND, None, wanted, fs_parent)
    assert (dev.put(KIND, np.frombuffer(wanted, np.uint8), np.frombuffer(fs_parent, np.uint8)) == capi.RF_OK).all()
    for fid, want_state in ((good, W.HIT), (other, W.READY)):
        g.set_slots([s for _, s in files], np.frombuffer(b"".join(f for f, _ in files), np.uint8))  # the ID unset again
        g.recompute(full=True)
        keys0 = node_keys()
        m.begin([0], ref, KIND, keys0)
        w.begin([0], dev, KIND, graph=g)
        compare(w, m)
        assert m.states.tolist() == [W.TODO, W.READY, W.DONE] and w.stats().looked_up == 1
        from_graph = results(w)
        w.begin([0], dev, KIND, keys=g.get_slots(key_slots))  # the same rows from the host
        assert results(w) == from_graph
        # the child finishes with this value: its file's slot is set ...
        g.set_slots([value_slot], np.frombuffer(fid, np.uint8))
        with pytest.raises(capi.RfError) as e:  # ... and while that change is pending a step is refused
            w.step([1], dev, KIND, graph=g)
        assert e.value.code == capi.RF_EPRECONDITION and results(w) == from_graph
        g.recompute(full=False)
        keys1 = node_keys()
        child.value.map["out"] = (fid, 3)
        child.done = True
        assert keys1[0][0] == parent.physical_digest() != keys0[0][0] and keys1[0][1] == keys0[0][1]
        child.done = False
        m.step([1], ref, KIND, keys1)
        w.step([1], dev, KIND, graph=g)
        compare(w, m)
        assert m.states[0] == want_state and w.stats().looked_up == 1 and w.stats().keys_probed == 2
        if want_state == W.HIT:
            assert m.hits[0] == (0, fs_parent, 0b01)
    # an object opened without key_slots cannot read a graph
    q = capi.EvalWave(ctx, dep_ptr, deps, flags, np.array(key_ptr, np.uint64))
    with pytest.raises(capi.RfError) as e:
        q.begin([0], dev, KIND, graph=g)
    assert e.value.code == capi.RF_EPRECONDITION
    q.close()
    w.close()
    g.close()
    dev.close()


# ---- 6. the top-down hand-over, determinism ---------------------------------------------
def _layered(widths):
    """Layer l has widths[l] nodes; each lists 1-3 nodes of the layer beneath."""
    rng = np.random.default_rng(11)
    starts = np.concatenate([[0], np.cumsum(widths)])
    dep_lists = []
    for l, wd in enumerate(widths):
        for _ in range(wd):
            if l + 1 == len(widths):
                dep_lists.append([])
            else:
                dep_lists.append((starts[l + 1] + rng.integers(0, widths[l + 1], size=rng.integers(1, 4))).tolist())
    return dep_lists, starts


@pytest.fixture(scope="module")
def big_case():
    """A layered graph with cached nodes at several depths, shared by the tests below."""
    widths = [3, 40, 300, 700, 300]
    dep_lists, starts = _layered(widths)
    n = int(starts[-1])
    flags = [W.F_CACHEABLE if i % 4 != 1 else 0 for i in range(n)]
    keys = hand_keys(flags, two=range(0, n, 3))
    cached = [i for i in range(3, n) if flags[i] and i % 5 in (0, 2)]
    return dep_lists, flags, keys, cached, list(range(int(starts[2])))  # the first two layers are the roots


def test_top_down_hand_over(ctx, big_case):
    """rf_eval_plan_run, then begin_states from the plan's device pointer: wave 0
    is the plan's READY list, and stepping to the end never looks anything up."""
    dep_lists, flags, keys, cached, roots = big_case
    h = Hand(ctx, dep_lists, flags, keys, cached=cached, second_only=cached[::3])
    ptr = np.zeros(len(dep_lists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(d) for d in dep_lists])
    deps = np.array([x for d in dep_lists for x in d], np.uint32)
    plan = capi.EvalPlan(ctx, ptr, deps, np.array(flags, np.uint8), P.key_arrays(keys)[0])
    plan.run(roots, h.dev, KIND, keys=h.flat)
    some_hits = plan.list(capi.RF_PLAN_HIT)[0][::7]
    plan.reject(some_hits, h.dev, KIND, keys=h.flat)  # rejects applied before the hand-over
    st = plan.states()
    assert all(c > 0 for c in plan.stats().counts[:4])
    for on_device in (True, False):
        h.m.begin_states(st)
        if on_device:
            h.w.begin_states(d_states=plan.states_device())
        else:
            h.w.begin_states(st)
        compare(h.w, h.m)
        ready = plan.list(capi.RF_PLAN_READY)[0]
        assert h.w.list(W.READY, W.LAST)[0].tobytes() == ready.tobytes() == h.w.list(W.READY)[0].tobytes()
        assert h.w.stats().mode == capi.RF_WAVE_MODE_TOPDOWN and h.w.stats().last_wave == len(ready)
        rng = np.random.default_rng(3)
        while h.open_nodes():
            open_ = np.array(h.open_nodes())
            done = open_[rng.random(len(open_)) < 0.5] if on_device else open_
            h.m.step(done)
            if on_device:
                h.w.step(done)  # no keys, no assoc: nothing is read
            else:
                h.w.step(done, h.dev, KIND, keys=h.flat)
            compare(h.w, h.m)
            assert h.w.stats().looked_up == 0 and h.w.stats().counts[W.HIT] == 0
        assert h.m.counts()[W.TODO] == 0 and all(h.m.states[r] == W.DONE for r in roots if st[r] != W.UNSEEN)
    # a wave object may take over its own states: they are copied first
    h.begin(roots)
    own = h.w.states()
    h.m.begin_states(own)
    h.w.begin_states(d_states=h.w.states_device())
    compare(h.w, h.m)
    plan.close()
    h.close()


def _evaluate(h, roots, split, on_step=None):
    """A whole bottom-up evaluation on the device alone; split(open nodes) picks
    what finishes in a step.  Returns results() after begin and after each step."""
    out = []
    h.w.begin(roots, h.dev, KIND, keys=h.flat)
    out.append(results(h.w))
    while True:
        open_ = np.concatenate([h.w.list(W.READY)[0], h.w.list(W.HIT)[0]])
        if not len(open_):
            return out
        h.w.step(split(np.sort(open_)), h.dev, KIND, keys=h.flat)
        out.append(results(h.w))
        if on_step:
            on_step(len(out))


def test_same_bytes_every_time(ctx, big_case):
    """The same evaluation twice, on a second stream with device keys, and over a
    table that grew and was compacted between steps gives identical bytes; a
    different split of the finished set into steps gives the same final states."""
    dep_lists, flags, keys, cached, roots = big_case
    h = Hand(ctx, dep_lists, flags, keys, cached=cached, second_only=cached[::3])

    def everything(open_):
        return open_
    first = _evaluate(h, roots, everything)
    assert len(first) >= 6 and first[1]["counts"][W.HIT] > 0
    # against the model once, so that the bytes compared below are the right ones
    h.begin(roots)
    h.to_the_end()
    assert results(h.w) == first[-1]
    assert _evaluate(h, roots, everything) == first
    # a caller's stream and device keys
    d_keys = capi.DeviceBuffer(ctx, h.flat.nbytes)
    d_keys.copy_from(h.flat)
    other = capi.Context(0, host_threads=0)
    again = []
    h.w.begin(roots, h.dev, KIND, d_keys=d_keys.ptr, stream=other.stream)
    again.append(results(h.w))
    while True:
        open_ = np.sort(np.concatenate([h.w.list(W.READY)[0], h.w.list(W.HIT)[0]]))
        if not len(open_):
            break
        h.w.step(open_, h.dev, KIND, d_keys=d_keys.ptr, stream=other.stream)
        again.append(results(h.w))
    other.close()
    d_keys.free()
    assert again == first
    # the table grows after begin and is compacted two steps later: the hits' values were copied at lookup time
    _, cap0 = h.dev.stats()
    extra = [C.fake_key(b"extra", i) for i in range(3 * cap0 // 4)]

    def churn(step):
        if step == 2:
            h.put(extra, [C.fake_key(b"extra value", i) for i in range(len(extra))])
            assert h.dev.stats()[1] > cap0
        if step == 4:
            h.put(extra[::2], [bytes(32)] * len(extra[::2]))
            h.dev.compact()
    assert _evaluate(h, roots, everything, on_step=churn) == first
    # another split of the same finished set: half of what is open per step, then the other half
    rng = np.random.default_rng(5)

    def half(open_):
        pick = open_[rng.random(len(open_)) < 0.5]
        return pick if len(pick) else open_[:1]
    split = _evaluate(h, roots, half)
    assert len(split) > len(first) and split[-1]["states"] == first[-1]["states"]
    assert split[-1]["counts"] == first[-1]["counts"]
    h.close()
