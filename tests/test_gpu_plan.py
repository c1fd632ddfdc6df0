"""The evaluation plan on the device (rf_eval_plan_*, k7_plan.hip) against its
CPU model (tests/plan_model.py: Eval.todo + Eval.lookup in top-down mode,
eval.go:902-955, 1163-1269): the states of every node, each list byte for
byte, and the counts -- for the reference's two behavioural flows, random
flows over every op, hand-built shapes at the kernel's edges, keys read from
a loaded graph, reject, list caps, and runs repeated on another stream and
over a table that grew and was compacted."""
import hashlib
import random

import numpy as np
import pytest

import plan_model as M
import reflow_oracle as O
from reflow_amd import capi

pytestmark = pytest.mark.gpu

KIND, OTHER_KIND = 0, 7


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


# ---- helpers ---------------------------------------------------------------------
class Tables:
    """The device assoc and the oracle's in-memory one, written together."""

    def __init__(self, ctx, capacity=1024):
        self.dev = capi.Assoc(ctx, capacity)
        self.ref = O.InmemoryAssoc()

    def put(self, kind, keys, vals):
        if not keys:
            return
        st = self.dev.put(kind, np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(vals), np.uint8))
        assert (st == capi.RF_OK).all()
        for k, v in zip(keys, vals):
            self.ref.put(kind, None, k, v)

    def close(self):
        self.dev.close()


def device_liveset(ctx, live):
    return None if live is None else capi.Bloom.load(ctx, live.m, live.k, live.words, live.length)


def open_plan(ctx, nodes, node_keys, invalid=(), key_slots=None):
    dep_ptr, deps = M.flow_csr(nodes)
    key_ptr, keys = M.key_arrays(node_keys)
    p = capi.EvalPlan(ctx, dep_ptr, deps, M.flow_flags(nodes, invalid), key_ptr, key_slots)
    return p, keys


def results(p):
    """Everything a plan reports, as bytes: states, the five lists, the counts."""
    out = {"states": p.states().tobytes(), "counts": list(p.stats().counts)}
    for state in range(5):
        out[state] = tuple(a.tobytes() for a in p.list(state))
    return out


def compare(p, want):
    st = p.states()
    assert st.tolist() == want.states.tolist()
    assert list(p.stats().counts) == want.counts()
    for state in range(5):
        nodes, which, vals, mask = p.list(state)
        wn, ww, wv, wm = want.list(state)
        assert nodes.dtype == np.uint32 and nodes.tobytes() == wn.tobytes(), state
        if state == M.HIT:
            assert which.tobytes() == ww.tobytes() and mask.tobytes() == wm.tobytes()
            assert vals.tobytes() == wv.tobytes()
    s = p.stats()
    assert s.rounds <= s.depth and s.n_nodes == len(want.states)


def fake_key(tag, i):
    return hashlib.sha256(b"%s %d" % (tag, i)).digest()


def hand_graph(dep_lists, cacheable):
    """OFlow nodes for a graph given as dep index lists: an OpExec where
    cacheable[i], else an OpMerge.  Their cache keys are made up (fake_key)."""
    nodes = [O.OFlow("OpExec" if c else "OpMerge") for c in cacheable]
    for f, d in zip(nodes, dep_lists):
        f.deps = [nodes[j] for j in d]
    return nodes


def hand_keys(cacheable, two=()):
    two = set(two)
    return [([fake_key(b"phys", i)] if i in two else []) + [fake_key(b"logical", i)] if c else []
            for i, c in enumerate(cacheable)]


def run_and_compare(ctx, nodes, node_keys, roots, tables, live=None, nce=False, invalid=()):
    p, keys = open_plan(ctx, nodes, node_keys, invalid)
    dl = device_liveset(ctx, live)
    p.run(roots, tables.dev, KIND, keys=keys, live=dl, no_cache_extern=nce)
    want = M.plan(nodes, roots, tables.ref, KIND, node_keys=node_keys, live=live, no_cache_extern=nce,
                  invalid=invalid)
    compare(p, want)
    if dl is not None:
        dl.close()
    return p, want


# ---- 1. the reference's behavioural flows ---------------------------------------------
def _cache(tables, nodes, which):
    for i in which:
        ks = nodes[i].cache_keys()
        tables.put(KIND, ks, [M.fileset_id(i)] * len(ks))


def test_cache_lookup_flow(ctx):
    """TestCacheLookup (test/evaltest/eval_test.go:174-230)."""
    nodes, ix = M.cache_lookup_flow()
    keys = [f.cache_keys() for f in nodes]
    t = Tables(ctx)
    _cache(t, nodes, [ix["extern"]])
    p, want = run_and_compare(ctx, nodes, keys, [ix["extern"]], t)
    assert want.states[ix["extern"]] == M.HIT and want.counts()[M.UNSEEN] == len(nodes) - 1
    assert p.stats().looked_up == 1 and p.stats().keys_probed == 1
    p.close()
    t.close()
    t = Tables(ctx)
    _cache(t, nodes, [ix["intern"]])
    p, want = run_and_compare(ctx, nodes, keys, [ix["extern"]], t)
    assert want.states[ix["groupby"]] == M.READY and want.states[ix["mapexec"]] == M.UNSEEN
    assert p.stats().looked_up == 2  # the extern and the intern
    p.close()
    t.close()


def test_no_cache_extern_flow(ctx):
    """TestNoCacheExtern (test/evaltest/eval_test.go:314-351), every key cached."""
    nodes, ix = M.no_cache_extern_flow()
    keys = [f.cache_keys() for f in nodes]
    t = Tables(ctx)
    _cache(t, nodes, range(len(nodes)))
    roots = [ix["top"], ix["clean_root"]]
    p, want = run_and_compare(ctx, nodes, keys, roots, t, nce=True)
    assert want.states[ix["clean"]] == M.HIT and want.states[ix["consumer"]] == M.TODO
    assert want.states[ix["extern"]] != M.HIT and want.states[ix["top"]] != M.HIT
    assert p.stats().looked_up == 2  # the clean exec and the intern; no dirty node, extern or root
    # the same plan object without NoCacheExtern, then with it again (the dirty bits are kept)
    dev_keys = M.key_arrays(keys)[1]
    p.run(roots, t.dev, KIND, keys=dev_keys)
    compare(p, M.plan(nodes, roots, t.ref, KIND, node_keys=keys))
    p.run(roots, t.dev, KIND, keys=dev_keys, no_cache_extern=True)
    compare(p, want)
    # the consumer stops being over an extern: set_flags on an EXTERN bit drops the kept bits
    e = ix["extern"]
    p.set_flags([e], [M.F_CACHEABLE])
    nodes[e].op = O.OP["OpExec"]
    try:
        p.run(roots, t.dev, KIND, keys=dev_keys, no_cache_extern=True)
        compare(p, M.plan(nodes, roots, t.ref, KIND, node_keys=keys, no_cache_extern=True))
    finally:
        nodes[e].op = O.OP["OpExtern"]
    p.close()
    t.close()


# ---- 2. random flows ------------------------------------------------------------------
# DAG seed -> the seed of the cache fill (random_case).  Seeds 1-5 are the
# suite's usual random flows; with the three highest-numbered nodes as roots and
# DONE taken from f.done (most of flowgen's nodes are done), their plans end
# after a handful of nodes, and only seed 2 has a fill under which every state
# occurs.  Seeds 6, 40, 58 and 118 were picked, with their fills, on the CPU
# from the model alone (the first fill seed in 0..149 that works), so that with
# and without the liveset every state occurs and some hit is found under its
# second key; COVERING lists the cases for which that is asserted.
FILL_SEED = {1: 0, 2: 22, 3: 0, 4: 0, 5: 0, 6: 3, 40: 2, 58: 2, 118: 2}
COVERING = (2, 6, 40, 58, 118)


_DAGS = {}


def random_dag_keys(seed):
    """flowgen.random_dag(seed, 200) without its synthetic root (which lists
    every node and would reach everything in one round), the three
    highest-numbered nodes as roots, and every node's cache keys."""
    if seed not in _DAGS:
        from flowgen import random_dag
        nodes = random_dag(seed, n=200)[1][:-1]
        _DAGS[seed] = (nodes, [len(nodes) - 1, len(nodes) - 2, len(nodes) - 3], M.cache_keys_of(nodes))
    return _DAGS[seed]


def random_case(seed, fill_seed):
    nodes, roots, keys = random_dag_keys(seed)
    rng = random.Random(fill_seed)
    puts, other, deleted = [], [], []
    for i, f in enumerate(nodes):
        if not keys[i] or rng.random() < 0.3:
            continue
        mode = rng.choice(["physical", "logical", "both", "neither"])
        if mode == "neither":
            other.append((keys[i][-1], fake_key(b"other kind", i)))  # cached under another kind only
            if rng.random() < 0.5:
                deleted.append(keys[i][0])                          # and put, then deleted
            continue
        ks = {"physical": keys[i][:1], "logical": keys[i][-1:], "both": keys[i]}[mode]
        for k in ks:
            puts.append((k, M.fileset_id(i)))
            other.append((k, fake_key(b"other kind", i)))
    invalid = sorted(rng.sample(range(len(nodes)), len(nodes) // 20))
    live_keys = [k for k, _ in puts if rng.random() < 0.8]
    return nodes, roots, keys, puts, other, deleted, invalid, live_keys


def fill(tables, puts, other, deleted):
    tables.put(KIND, [k for k, _ in puts], [v for _, v in puts])
    tables.put(OTHER_KIND, [k for k, _ in other], [v for _, v in other])
    tables.put(KIND, deleted, [fake_key(b"short-lived", 0)] * len(deleted))
    tables.put(KIND, deleted, [bytes(32)] * len(deleted))


def model_covers_everything(want):
    return all(c > 0 for c in want.counts()) and any(w == 1 for w, _, _ in want.hits.values())


@pytest.mark.parametrize("with_liveset", [False, True])
@pytest.mark.parametrize("seed", sorted(FILL_SEED))
def test_random_flows(ctx, seed, with_liveset):
    nodes, roots, keys, puts, other, deleted, invalid, live_keys = random_case(seed, FILL_SEED[seed])
    t = Tables(ctx)
    fill(t, puts, other, deleted)
    live = M.Liveset(live_keys) if with_liveset else None
    p, want = run_and_compare(ctx, nodes, keys, roots, t, live=live, invalid=invalid)
    if seed in COVERING:
        assert model_covers_everything(want), want.counts()
    s = p.stats()
    if with_liveset:
        assert s.keys_filtered > 0 or seed not in COVERING
    else:
        assert s.keys_filtered == 0 and s.keys_probed == sum(len(keys[i]) for i in range(len(nodes))
                                                              if want.states[i] == M.HIT or _looked_up_miss(
                                                                  nodes, keys, invalid, want, i))
    p.close()
    t.close()


def _looked_up_miss(nodes, keys, invalid, want, i):
    return (want.states[i] in (M.TODO, M.READY) and M.flow_flags([nodes[i]])[0] & M.F_CACHEABLE and
            i not in invalid and len(keys[i]) > 0)


# ---- 3. shape edges -------------------------------------------------------------------
def _cache_every(tables, node_keys, which_nodes, second_only=()):
    ks, vs = [], []
    for i in which_nodes:
        for k in (node_keys[i][-1:] if i in second_only else node_keys[i]):
            ks.append(k)
            vs.append(M.fileset_id(i))
    tables.put(KIND, ks, vs)


def test_degrees(ctx):
    """Deps of degree 0, 1, 63, 64, 65, 129 and 1000, one with a dep listed
    twice, under a root that misses; every third leaf is cached."""
    degs = [0, 1, 63, 64, 65, 129, 1000]
    n_mid = len(degs)
    leaves0 = 1 + n_mid
    n = leaves0 + 1100
    rng = np.random.default_rng(5)
    dep_lists = [list(range(1, 1 + n_mid))]
    for d in degs:
        dl = (leaves0 + rng.permutation(1100)[:d]).tolist()
        if d >= 63:
            dl[d // 2] = dl[0]  # a duplicated dep
        dep_lists.append(dl)
    dep_lists += [[] for _ in range(1100)]
    cacheable = [True] * n
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable, two=range(leaves0, n, 2))
    t = Tables(ctx)
    hits = list(range(leaves0, n, 3))
    _cache_every(t, keys, hits, second_only=set(hits[::2]))
    p, want = run_and_compare(ctx, nodes, keys, [0], t)
    assert want.counts()[M.HIT] > 300 and want.states[1] == M.READY
    assert any(w == 1 for w, _, _ in want.hits.values())
    p.close()
    t.close()


def _layered(widths, cover=True):
    """Layer l has widths[l] nodes; each node lists 1-3 nodes of the layer
    beneath (with cover, the first node of a layer lists all of it, so every
    node is reached unless a hit is in the way)."""
    rng = np.random.default_rng(11)
    starts = np.concatenate([[0], np.cumsum(widths)])
    dep_lists = []
    for l, w in enumerate(widths):
        for j in range(w):
            if l + 1 == len(widths):
                dep_lists.append([])
            elif j == 0 and cover:
                dep_lists.append(list(range(starts[l + 1], starts[l + 2])))
            else:
                dep_lists.append((starts[l + 1] + rng.integers(0, widths[l + 1], size=rng.integers(1, 4))).tolist())
    return dep_lists, starts


def test_layer_widths(ctx):
    widths = [1, 63, 64, 65, 255, 256, 257]
    dep_lists, starts = _layered(widths)
    n = int(starts[-1])
    cacheable = [i % 2 == 0 for i in range(n)]
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable)
    t = Tables(ctx)
    _cache_every(t, keys, [i for i in range(int(starts[4]), n) if cacheable[i] and i % 3 == 0])
    p, want = run_and_compare(ctx, nodes, keys, [0], t)
    assert p.stats().depth == len(widths) and p.stats().rounds >= len(widths)
    p.close()
    t.close()


def test_layer_wider_than_a_round_launch(ctx):
    """One layer wider than the round kernel's grid has lanes: the grid strides."""
    probe = capi.EvalPlan(ctx, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint8),
                          np.zeros(2, np.uint64))
    max_lanes = 1024 * 256  # the largest grid: read back below
    probe.close()
    width = max_lanes + 1000
    n = 1 + width + 3
    dep_lists = [list(range(1, 1 + width))] + [[1 + width + (i % 3)] for i in range(width)] + [[], [], []]
    cacheable = [False] * n
    for i in range(1, 1 + width, 997):
        cacheable[i] = True
    cacheable[-1] = cacheable[-2] = True
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable)
    t = Tables(ctx)
    _cache_every(t, keys, [i for i in range(1, 1 + width, 2 * 997)] + [n - 1])
    p, want = run_and_compare(ctx, nodes, keys, [0], t)
    s = p.stats()
    assert s.round_lanes == max_lanes and width > s.round_lanes
    assert want.counts()[M.UNSEEN] == 0 and want.counts()[M.HIT] > 100
    p.close()
    t.close()


def test_chain_longer_than_three_batches(ctx):
    probe = capi.EvalPlan(ctx, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint8),
                          np.zeros(2, np.uint64))
    batch = probe.stats().round_batch
    probe.close()
    n = 3 * batch + 1
    dep_lists = [[i + 1] for i in range(n - 1)] + [[]]
    cacheable = [True] * n
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable)
    t = Tables(ctx)
    p, want = run_and_compare(ctx, nodes, keys, [0], t)  # nothing cached: the whole chain
    s = p.stats()
    assert s.depth == n and s.rounds <= s.depth and s.rounds >= n and want.counts()[M.READY] == 1
    p.close()
    _cache_every(t, keys, [n - 2])
    p, want = run_and_compare(ctx, nodes, keys, [0], t)
    assert want.states[n - 1] == M.UNSEEN and want.states[n - 3] == M.READY
    p.close()
    t.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_list_tile_edges(ctx, delta):
    probe = capi.EvalPlan(ctx, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint8),
                          np.zeros(2, np.uint64))
    tile = probe.stats().list_tile
    probe.close()
    n = tile + delta
    dep_lists = [list(range(1, n))] + [[] for _ in range(n - 1)]
    cacheable = [False] + [True] * (n - 1)
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable)
    t = Tables(ctx)
    _cache_every(t, keys, [1, 2, n - 2, n - 1] + list(range(5, n, 7)))
    p, want = run_and_compare(ctx, nodes, keys, [0], t)
    assert want.states[n - 1] == M.HIT and want.states[n - 3 if (n - 3 - 5) % 7 else n - 4] == M.READY
    p.close()
    t.close()


def test_roots_twice_done_root_and_nothing(ctx):
    dep_lists = [[2, 3], [3, 4], [5], [5], [], []]
    cacheable = [True, False, True, True, True, True]
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable)
    t = Tables(ctx)
    _cache_every(t, keys, [3])
    p, want = run_and_compare(ctx, nodes, keys, [0, 1, 0, 1, 1], t)   # roots given twice
    assert want.states.tolist() == [M.TODO, M.TODO, M.TODO, M.HIT, M.READY, M.READY]
    p.close()
    nodes[1].done = True                                              # a done root: DONE, not expanded
    nodes[5].done = True                                              # a done dep: DONE, satisfies node 2
    p, want = run_and_compare(ctx, nodes, keys, [1, 0], t)
    assert want.states.tolist() == [M.TODO, M.DONE, M.READY, M.HIT, M.UNSEEN, M.DONE]
    # no roots: nothing is reached, every list but UNSEEN is empty
    p.run([], t.dev, KIND, keys=M.key_arrays(keys)[1])
    assert p.states().tolist() == [M.UNSEEN] * 6 and list(p.stats().counts) == [6, 0, 0, 0, 0]
    assert p.list(M.UNSEEN)[0].tolist() == list(range(6)) and p.stats().rounds == 0
    p.close()
    # no nodes at all
    empty = capi.EvalPlan(ctx, np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8),
                          np.zeros(0, np.uint64))
    empty.run([], t.dev, KIND)
    assert empty.stats().depth == 0 and list(empty.stats().counts) == [0] * 5
    assert all(len(empty.list(s)[0]) == 0 for s in range(5)) and len(empty.states()) == 0
    empty.close()
    t.close()


def test_open_refuses_bad_graphs(ctx):
    def refused(dep_lists, key_counts=None):
        n = len(dep_lists)
        ptr = np.zeros(n + 1, np.uint64)
        ptr[1:] = np.cumsum([len(d) for d in dep_lists])
        deps = np.array([x for d in dep_lists for x in d], np.uint32)
        kp = np.zeros(n + 1, np.uint64)
        kp[1:] = np.cumsum(key_counts or [1] * n)
        with pytest.raises(capi.RfError) as e:
            capi.EvalPlan(ctx, ptr, deps, np.ones(n, np.uint8), kp)
        assert e.value.code == capi.RF_EINVAL
        return str(e.value)
    assert "cycle" in refused([[1], [0]])
    assert "out of range" in refused([[5], []])
    assert "cache keys" in refused([[1], []], [capi.RF_PLAN_MAX_KEYS + 1, 1])
    ok = capi.EvalPlan(ctx, np.array([0, 1, 1], np.uint64), np.array([1], np.uint32), np.ones(2, np.uint8),
                       np.array([0, capi.RF_PLAN_MAX_KEYS, capi.RF_PLAN_MAX_KEYS], np.uint64))
    assert ok.stats().depth == 2
    with pytest.raises(capi.RfError) as e:  # a root out of range
        ok.run([2], capi.Assoc(ctx), KIND, keys=np.zeros((capi.RF_PLAN_MAX_KEYS, 32), np.uint8))
    assert e.value.code == capi.RF_EINVAL
    ok.close()


# ---- 4. keys from a graph -------------------------------------------------------------
def _filesets(f):
    out, stack = [], [f.value] if f.value is not None else []
    while stack:
        v = stack.pop()
        out.append(v)
        if v.list:
            stack.extend(v.list)
    return out


def _replace_file(nodes, old, new):
    for f in nodes:
        for v in _filesets(f):
            for path, (fid, size) in list((v.map or {}).items()):
                if fid == old:
                    v.map[path] = (new, size)


def test_keys_from_a_graph(ctx):
    from flowgen import random_dag
    from lowering import Lowerer
    nodes = random_dag(10, n=80)[1][:-1]
    for f in nodes:
        f.done = f.done and f.op not in (O.OP["OpExec"], O.OP["OpExtern"])  # leave the cacheable ones to plan
    listed = {id(d) for f in nodes for d in f.deps}
    roots = [i for i, f in enumerate(nodes) if id(f) not in listed]  # the nodes nobody depends on
    low = Lowerer(file_slots=True)
    key_ptr, key_slots = [0], []
    for f in nodes:
        ps = low.lower_physical(f)
        if ps is not None:
            key_slots.append(ps)
        key_slots.append(low.lower(f))
        key_ptr.append(len(key_slots))
    key_slots = np.array(key_slots, np.uint32)
    g = capi.Graph.from_arrays(ctx, low.L.arrays())
    files = list(low.L.file_slot.items())
    g.set_slots([s for _, s in files], np.frombuffer(b"".join(fid for fid, _ in files), np.uint8))

    dep_ptr, deps = M.flow_csr(nodes)
    p = capi.EvalPlan(ctx, dep_ptr, deps, M.flow_flags(nodes), np.array(key_ptr, np.uint64), key_slots)
    t = Tables(ctx)
    with pytest.raises(capi.RfError) as e:  # never recomputed
        p.run(roots, t.dev, KIND, graph=g)
    assert e.value.code == capi.RF_EPRECONDITION
    g.recompute(full=True)

    def node_keys():
        rows = g.get_slots(key_slots)
        return [[rows[r].tobytes() for r in range(key_ptr[i], key_ptr[i + 1])] for i in range(len(nodes))]
    keys0 = node_keys()
    assert keys0 == M.cache_keys_of(nodes)  # the lowering's slots are the oracle's cache keys
    cached = [i for i, f in enumerate(nodes) if f.op in (O.OP["OpExec"], O.OP["OpIntern"]) and i % 3]
    _cache_every(t, keys0, cached)
    want0 = M.plan(nodes, roots, t.ref, KIND, node_keys=keys0)
    p.run(roots, t.dev, KIND, graph=g)
    compare(p, want0)
    from_graph = results(p)
    p.run(roots, t.dev, KIND, keys=g.get_slots(key_slots))
    assert results(p) == from_graph and want0.counts()[M.HIT] > 0
    # one file changes -- the first one that moves a key some hit was found under
    for fid, slot in files:
        new_id = O.sha256(fid + b" v2")
        _replace_file(nodes, fid, new_id)
        keys1 = M.cache_keys_of(nodes)
        if any(keys1[i][w] != keys0[i][w] for i, (w, _, _) in want0.hits.items()):
            break
        _replace_file(nodes, new_id, fid)
    else:
        raise AssertionError("no file moves a hit's key")
    # pending until the step: refused, and the last plan stays in place
    g.set_slots([slot], np.frombuffer(new_id, np.uint8))
    with pytest.raises(capi.RfError) as e:
        p.run(roots, t.dev, KIND, graph=g)
    assert e.value.code == capi.RF_EPRECONDITION
    assert results(p) == from_graph
    g.recompute(full=False)
    assert node_keys() == keys1
    moved = [i for i in range(len(nodes)) if keys1[i] != keys0[i]]
    want1 = M.plan(nodes, roots, t.ref, KIND, node_keys=keys1)
    p.run(roots, t.dev, KIND, graph=g)
    compare(p, want1)
    # a node whose every key moved now misses; the hit above it is gone
    assert all(want1.states[i] != M.HIT for i in moved if not set(keys1[i]) & set(keys0[i]))
    assert want1.states.tolist() != want0.states.tolist()
    # a plan opened without key_slots cannot read a graph
    q = capi.EvalPlan(ctx, dep_ptr, deps, M.flow_flags(nodes), np.array(key_ptr, np.uint64))
    with pytest.raises(capi.RfError) as e:
        q.run(roots, t.dev, KIND, graph=g)
    assert e.value.code == capi.RF_EPRECONDITION
    q.close()
    p.close()
    g.close()
    t.close()


# ---- 5. reject, caps, determinism -------------------------------------------------------
@pytest.fixture(scope="module")
def big_case(ctx):
    """A layered graph with hits at several depths, shared by the tests below."""
    widths = [3, 40, 300, 700, 300]
    dep_lists, starts = _layered(widths, cover=False)
    n = int(starts[-1])
    cacheable = [i % 4 != 1 for i in range(n)]
    nodes = hand_graph(dep_lists, cacheable)
    keys = hand_keys(cacheable, two=range(0, n, 3))
    t = Tables(ctx)
    cached = [i for i in range(3, n) if cacheable[i] and i % 5 in (0, 2)]
    _cache_every(t, keys, cached, second_only=set(cached[::3]))
    yield nodes, keys, list(range(int(starts[2]))), t, starts  # the first two layers are the roots
    t.close()


def test_reject(ctx, big_case):
    nodes, keys, roots, t, starts = big_case
    p, want = run_and_compare(ctx, nodes, keys, roots, t)
    idx = {id(f): i for i, f in enumerate(nodes)}
    hits = [int(i) for i in want.list(M.HIT)[0]]
    # a hit with hits and unseen nodes beneath it, a hit in the last layer, and one more
    def beneath(i):
        return {want.states[idx[id(d)]] for d in nodes[i].deps}
    deep = next(i for i in hits if M.UNSEEN in beneath(i) and any(
        keys[idx[id(d)]] and t.ref.get(KIND, keys[idx[id(d)]][-1]) for d in nodes[i].deps))
    rejected = [deep, hits[-1], hits[len(hits) // 2], deep]
    dev_keys = M.key_arrays(keys)[1]
    p.reject(rejected, t.dev, KIND, keys=dev_keys)
    want_r = M.reject(nodes, roots, t.ref, KIND, rejected, node_keys=keys)
    compare(p, want_r)
    assert want_r.counts()[M.HIT] != want.counts()[M.HIT] and want_r.states[deep] in (M.TODO, M.READY)
    # the same states from a fresh run with those nodes invalid
    q, _ = run_and_compare(ctx, nodes, keys, roots, t, invalid=sorted(set(rejected)))
    assert results(q) == results(p)
    q.close()
    # a second reject goes on from the first
    more = [int(want_r.list(M.HIT)[0][0])]
    p.reject(more, t.dev, KIND, keys=dev_keys)
    compare(p, M.reject(nodes, roots, t.ref, KIND, rejected + more, node_keys=keys))
    # a node that is no hit: refused, nothing changes
    before = results(p)
    todo = int(p.list(M.TODO)[0][0])
    with pytest.raises(capi.RfError) as e:
        p.reject([int(p.list(M.HIT)[0][0]), todo], t.dev, KIND, keys=dev_keys)
    assert e.value.code == capi.RF_EINVAL and results(p) == before
    p.close()


def test_list_caps(ctx, big_case):
    nodes, keys, roots, t, _ = big_case
    p, want = run_and_compare(ctx, nodes, keys, roots, t)
    for state in (M.HIT, M.READY):
        full = p.list(state)
        found = len(full[0])
        assert found > 10 and p.count(state) == found
        exact = p.list(state, cap=found, poison=0xAB)
        carried = 4 if state == M.HIT else 1  # which, value and found mask are written for hits only
        assert all(a.tobytes() == b.tobytes() for a, b in zip(exact[:carried], full[:carried]))
        with pytest.raises(capi.RfError) as e:
            p.list(state, cap=found - 1, poison=0xAB)
        assert e.value.code == capi.RF_EINVAL and e.value.needed == found
        nodes_b, which_b, vals_b, kf_b = e.value.buffers
        assert nodes_b[found - 1:].tobytes() == b"\xab" * 4 * len(nodes_b[found - 1:])
        for buf in (which_b, vals_b, kf_b):
            assert (buf[found - 1:] == 0xAB).all()
    # the device form: ranks below cap are written, the count is whole
    cap = 7
    d_nodes, d_which, d_vals = capi.DeviceBuffer(ctx, 4 * 64), capi.DeviceBuffer(ctx, 64), capi.DeviceBuffer(ctx, 32 * 64)
    d_kf, d_n = capi.DeviceBuffer(ctx, 64), capi.DeviceBuffer(ctx, 8)
    for b in (d_nodes, d_which, d_vals, d_kf):
        b.fill(0xAB)
    p.list_device(M.HIT, cap, d_nodes.ptr, d_which.ptr, d_vals.ptr, d_kf.ptr, d_n.ptr)
    ctx.sync()
    wn, ww, wv, wm = want.list(M.HIT)
    assert d_n.to_numpy(np.uint64)[0] == len(wn)
    assert d_nodes.to_numpy(np.uint32)[:cap].tobytes() == wn[:cap].tobytes()
    assert (d_nodes.to_numpy(np.uint32)[cap:] == 0xABABABAB).all()
    assert d_which.to_numpy()[:cap].tobytes() == ww[:cap].tobytes() and (d_which.to_numpy()[cap:] == 0xAB).all()
    assert d_kf.to_numpy()[:cap].tobytes() == wm[:cap].tobytes() and (d_kf.to_numpy()[cap:] == 0xAB).all()
    assert d_vals.to_numpy()[:32 * cap].tobytes() == wv[:cap].tobytes() and (d_vals.to_numpy()[32 * cap:] == 0xAB).all()
    for b in (d_nodes, d_which, d_vals, d_kf, d_n):
        b.free()
    p.close()


def test_same_bytes_every_time(ctx, big_case):
    """Two runs, a run on a second stream with device keys, and runs after the
    table grew and after it was compacted give identical bytes."""
    nodes, keys, roots, t, _ = big_case
    p, want = run_and_compare(ctx, nodes, keys, roots, t)
    first = results(p)
    dev_keys = M.key_arrays(keys)[1]
    p.run(roots, t.dev, KIND, keys=dev_keys)
    assert results(p) == first
    d_keys = capi.DeviceBuffer(ctx, dev_keys.nbytes)
    d_keys.copy_from(dev_keys)
    other = capi.Context(0, host_threads=0)  # a caller's stream
    p.run(roots, t.dev, KIND, d_keys=d_keys.ptr, stream=other.stream)
    other.close()
    assert results(p) == first
    # growth: many more keys under this kind (none of them a node's), some deleted again
    _, cap0 = t.dev.stats()
    extra = [fake_key(b"extra", i) for i in range(3 * cap0 // 4)]
    t.put(KIND, extra, [fake_key(b"extra value", i) for i in range(len(extra))])
    assert t.dev.stats()[1] > cap0
    p.run(roots, t.dev, KIND, keys=dev_keys)
    assert results(p) == first
    # the hits' values were copied at lookup time: a list after the table moved is still right
    t.put(KIND, extra[::2], [bytes(32)] * len(extra[::2]))
    t.dev.compact()
    assert results(p) == first
    p.run(roots, t.dev, KIND, d_keys=d_keys.ptr)
    assert results(p) == first
    compare(p, want)
    d_keys.free()
    p.close()
