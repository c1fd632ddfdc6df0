"""The GC liveset on the device (rf_liveset_*, k8_live.hip) against its CPU
model (tests/live_model.py: Eval.collect, eval.go:791-868): the states of
every node, the three lists, every counter of rf_liveset_stats, the filter's
(m, k, length) and every one of its words -- for TestGC's flow stage by stage,
random flows over every op, a deep layered graph, hand-built shapes at the
kernels' edges (degrees, list tiles, row counts), updates between runs, the
borrowed filter through the rf_bloom_* calls, and the refusals."""
import ctypes
import random

import numpy as np
import pytest

import flowgen
import live_model as M
import reflow_oracle as O
from reflow_amd import capi

pytestmark = pytest.mark.gpu

TILE = capi.RF_LIVE_LIST_TILE


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


# ---- helpers ---------------------------------------------------------------------
def fid(rng) -> bytes:
    return rng.bytes(32)


def fileset(rows):
    """A Map of the given (id, size) rows, in order (paths are distinct, rows need not be)."""
    return O.OFileset(map={"p%06d" % i: r for i, r in enumerate(rows)})


def node(deps=(), rows=None, done=None):
    """A plain node; rows: its Fileset value's rows (done unless told otherwise)."""
    f = O.OFlow("OpMerge", list(deps))
    if rows is not None:
        f.value = fileset(rows)
        f.done = True if done is None else done
    elif done:
        f.done = True
    return f


class Session:
    """One rf_liveset and everything the model and plain bookkeeping say it must report."""

    def __init__(self, ctx, nodes):
        self.ctx, self.nodes = ctx, nodes
        self.L = capi.GcLiveset(ctx, *M.live_csr(nodes))
        self.prev, self.maxlive, self.rows, self.stale = None, 0, 0, 0
        self.cur = {}  # node -> rows of its current value
        self.push(range(len(nodes)))

    def push(self, which):
        """Send the listed nodes' present state: a value (set) or none (clear)."""
        which = [int(i) for i in which]
        nd, ct, ids, sz = M.value_arrays(self.nodes, which)
        if len(nd):
            self.L.set_values(nd, ct, ids, sz)
        for i, c in zip(nd.tolist(), ct.tolist()):
            self.stale += self.cur.pop(i, 0)
            self.cur[i] = c
            self.rows += c
        gone = [i for i in which if not M.has_value(self.nodes[i]) and i in self.cur]
        if gone:
            self.L.clear_values(gone)
            self.stale += sum(self.cur.pop(i) for i in gone)

    def run(self, roots, writers=(), stream=None):
        st = self.L.run(roots, writers, stream=stream)
        want = M.live(self.nodes, roots, writers, prev=self.prev)
        self.maxlive = max(self.maxlive, want.livebytes)
        compare(self.L, st, want)
        assert (st.maxlivebytes, st.arena_rows, st.stale_rows) == (self.maxlive, self.rows, self.stale)
        self.prev = want
        return st, want

    def close(self):
        self.L.close()


def compare(L, st, want):
    assert L.states().tolist() == want.states.tolist()
    assert st.n_nodes == len(want.states) and list(st.counts) == want.counts()
    for state in range(3):
        got = L.list(state)
        assert got.dtype == np.uint32 and got.tobytes() == want.list(state).tobytes(), state
    assert (st.contributions, st.nlive_est, st.nlive, st.livebytes) == \
        (len(want.contributions), want.nlive_est, want.nlive, want.livebytes)
    assert (st.m, st.k, st.changed) == (want.m, want.k, int(want.changed))
    b = L.filter()
    m, k, length, nw = b.params()
    assert (m, k, length, nw) == (want.m, want.k, want.length, len(want.words))
    assert b.words().tobytes() == want.words.tobytes()
    assert st.device_bytes > 0


# ---- TestGC ------------------------------------------------------------------------
def test_gc_flow_stage_by_stage(ctx):
    nodes, ix = M.gc_flow()
    s = Session(ctx, nodes)
    ids, sizes = M.gc_objects()
    root = [ix["pullup"]]
    for stage in range(4):
        M.gc_stage(nodes, ix, stage)
        s.push(range(len(nodes)) if stage else [])
        st, want = s.run(root)
        assert st.changed == 1
        words = s.L.filter().words().tobytes()
        st2, _ = s.run(root)  # nothing happened in between: Repository.Collect is not due
        assert st2.changed == 0 and s.L.filter().words().tobytes() == words
    assert (st.m, st.k, st.nlive) == (101, 11, 7)
    dead, dead_bytes = s.L.filter().collect(ids, sizes)
    assert dead.tolist() == [7] and dead_bytes == len("unrooted")  # exactly `unrooted` is collected
    s.close()


# ---- random flows --------------------------------------------------------------------
@pytest.mark.parametrize("seed,n", [(1, 60), (2, 150), (3, 300), (4, 300)])
def test_random_dags(ctx, seed, n):
    root, _ = flowgen.random_dag(seed, n)
    nodes = M.all_nodes(root)
    s = Session(ctx, nodes)
    rng = random.Random(seed)
    _, want = s.run([0])
    assert want.counts()[M.VALUE] > 0
    for _ in range(2):
        roots = [rng.randrange(len(nodes)) for _ in range(5)]
        writers = [rng.randrange(len(nodes)) for _ in range(rng.randint(0, 6))]
        s.run(roots, writers)
    s.close()


# ---- a deep layered graph ------------------------------------------------------------
@pytest.fixture(scope="module")
def layered():
    rng = np.random.default_rng(12)
    layers, width = 12, 1700
    nodes = [node()]
    prev = [nodes[0]]
    for depth in range(1, layers):
        cur = []
        for _ in range(width):
            rows = None
            if rng.random() < 0.12:  # a value at any depth: what lies beneath only it stays unseen
                rows = [(fid(rng), int(rng.integers(0, 1 << 20))) for _ in range(int(rng.integers(0, 4)))]
            cur.append(node(rows=rows))
        for f in prev:  # (the root fans out, so that the walk is wide as well as deep)
            f.deps = [cur[int(j)] for j in rng.integers(0, width, size=40 if depth == 1 else int(rng.integers(1, 4)))]
        nodes.extend(cur)
        prev = cur
    return nodes


def test_layered_graph_takes_many_rounds(ctx, layered):
    s = Session(ctx, layered)
    st, want = s.run([0])
    assert st.n_nodes > 18000
    assert capi.RF_LIVE_ROUND_BATCH < st.rounds <= 12 + capi.RF_LIVE_ROUND_BATCH
    unseen_values = [i for i in want.list(M.UNSEEN) if M.has_value(layered[i])]
    assert len(unseen_values) > 100 and want.counts()[M.VALUE] > 100  # values beneath values stay unseen
    first = (s.L.states().tobytes(), s.L.filter().words().tobytes())
    st2, _ = s.run([0])
    assert st2.changed == 0 and (s.L.states().tobytes(), s.L.filter().words().tobytes()) == first
    s.close()


# ---- degrees ---------------------------------------------------------------------------
def test_degree_edges(ctx):
    rng = np.random.default_rng(5)
    leaves = [node(rows=[(fid(rng), i)]) for i in range(200)]
    fans = [node(leaves[:d]) for d in (0, 1, 63, 64, 65, 200)]
    twice = node([leaves[7], leaves[7], leaves[8], leaves[7]])            # an edge listed twice
    below = node(rows=[(fid(rng), 1)])
    done_no_value = node([below], done=True)                              # Done, no Fileset: expanded
    valued_root = node([node(rows=[(fid(rng), 2)])], rows=[(fid(rng), 3)])  # a root that holds a value
    top = node(fans + [twice, done_no_value])
    nodes = M.all_nodes(node([top, valued_root]))
    ix = {id(f): i for i, f in enumerate(nodes)}
    s = Session(ctx, nodes)
    _, want = s.run([ix[id(top)]])
    assert want.states[ix[id(done_no_value)]] == M.WALKED and want.states[ix[id(below)]] == M.VALUE
    assert want.counts()[M.VALUE] == 201
    for f in fans:  # each fan alone: the narrow and the whole-wave path
        s.run([ix[id(f)]])
    _, want = s.run([ix[id(valued_root)], ix[id(valued_root)]])
    assert want.counts() == [len(nodes) - 1, 0, 1]
    s.close()


# ---- list tiles --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_list_tiling(ctx, n):
    rng = np.random.default_rng(n)
    hub = n // 2
    nodes = [node() for _ in range(n)]
    for i in range(n):
        if i != hub and (i % TILE in (0, 1, TILE - 2, TILE - 1) or i == n - 1 or rng.random() < 0.3):
            nodes[i] = node(rows=[(fid(rng), i)] * int(rng.integers(0, 3)))
    nodes[hub].deps = [nodes[i] for i in range(n) if i != hub and i % 7 != 3]  # some stay unseen
    s = Session(ctx, nodes)
    _, want = s.run([hub])
    got = want.list(M.VALUE).tolist()
    assert 0 in got and TILE - 2 in got and (n <= TILE or TILE in got)
    for state in range(3):  # the cap rule of rf_eval_plan_list
        found = len(want.list(state))
        assert s.L.count(state) == found
        if found > 1:
            with pytest.raises(capi.RfError) as e:
                s.L.list(state, cap=found - 1, poison=0xAB)
            assert e.value.code == capi.RF_EINVAL and e.value.needed == found
            assert (e.value.buffer == 0xABABABAB).all()  # nothing is written when the buffer is short
            exact = s.L.list(state, cap=found + 3, poison=0xAB)
            assert exact.tobytes() == want.list(state).tobytes()
    s.close()


# ---- rows ------------------------------------------------------------------------------------
def test_row_edges(ctx):
    rng = np.random.default_rng(9)
    shared = (fid(rng), 77)
    two_sizes = fid(rng)
    sized = [node(rows=[(fid(rng), int(rng.integers(0, 1 << 40))) for _ in range(c)])
             for c in (0, 1, 63, 64, 65, 255, 256, 257)]
    big_rows = [(fid(rng), int(rng.integers(0, 1 << 30))) for _ in range(60000)]
    big_rows += [big_rows[int(j)] for j in rng.integers(0, 60000, size=10000)]  # 10,000 repeat earlier pairs
    big = node(rows=[big_rows[int(j)] for j in rng.permutation(70000)])
    a = node(rows=[shared, (two_sizes, 5), (two_sizes, 6), shared])  # one ID with two sizes; a pair twice
    b = node(rows=[shared, (fid(rng), -3)])                           # the same file in a second value
    lone = node(rows=[(fid(rng), 9)] * 3)                             # reached by no root
    plain = node()
    top = node(sized + [big, a, b, plain])
    nodes = [top] + sized + [big, a, b, plain, lone]
    ix = {id(f): i for i, f in enumerate(nodes)}
    s = Session(ctx, nodes)
    st, want = s.run([0])
    assert want.nlive_est == 961 + 70000 + 4 + 2 and want.nlive == 961 + 60000 + 3 + 2
    # a writer on the frontier, a writer listed twice, a writer without a value
    st, want = s.run([0], [ix[id(a)], ix[id(lone)], ix[id(lone)], ix[id(plain)]])
    assert st.contributions == 11 + 4 and want.nlive == 961 + 60000 + 3 + 2 + 3 + 1 + 1
    # unreached writers only: an empty frontier
    st, want = s.run([], [ix[id(lone)], ix[id(b)]])
    assert want.counts() == [len(nodes), 0, 0] and (st.nlive_est, st.nlive) == (5, 3)
    s.close()


def test_all_empty(ctx):
    nodes = M.all_nodes(node([node(), node(rows=[])]))
    s = Session(ctx, nodes)
    for roots, writers in (([0], []), ([], []), ([0], [1, 2])):
        st, want = s.run(roots, writers)
        assert (st.m, st.k, st.nlive_est, st.nlive, st.livebytes) == (64, 1, 0, 0, 0)
        b = s.L.filter()
        assert b.params()[:3] == (64, 1, 64) and not b.words().any()
        rng = np.random.default_rng(1)
        assert not b.probe(rng.integers(0, 256, size=32 * 100, dtype=np.uint8)).any()
    s.close()


# ---- updates -----------------------------------------------------------------------------------
def test_updates_between_runs(ctx):
    rng = np.random.default_rng(21)

    def rows(c):
        return [(fid(rng), int(rng.integers(0, 1000))) for _ in range(c)]
    leaves = [node(rows=rows(3)) for _ in range(6)]
    mid = [node(leaves[0:3]), node(leaves[2:6])]
    top = node(mid)
    nodes = [top] + mid + leaves
    s = Session(ctx, nodes)
    st, want = s.run([0])
    assert want.counts() == [0, 3, 6]
    # a frontier-side node finishes: its subtree turns unseen, the liveset changes
    mid[0].done, mid[0].value = True, fileset(rows(2))
    s.push([1])
    st, want = s.run([0])
    assert st.changed == 1 and want.states.tolist() == [M.WALKED, M.VALUE, M.WALKED] + [M.UNSEEN] * 2 + [M.VALUE] * 4
    # replacing a value drops its old rows from every count
    leaves[5].value = fileset(rows(1))
    s.push([8])
    st, want = s.run([0])
    assert st.changed == 1 and st.nlive_est == 2 + 3 * 3 + 1 and st.stale_rows == 3
    # a node listed twice in one call keeps its last value
    nd, ct, ids, sz = M.value_arrays(nodes, [8])
    other = np.frombuffer(fid(rng) * 2, np.uint8)
    s.L.set_values([8, 8], [2, int(ct[0])], np.concatenate([other, ids.reshape(-1)]), np.concatenate([[1, 2], sz]))
    s.stale += s.cur[8] + 2
    s.rows += 2 + int(ct[0])
    st, want = s.run([0])
    assert st.changed == 0
    # no longer done: the node is expanded again
    mid[0].done, mid[0].value = False, None
    s.push([1])
    st, want = s.run([0])
    assert st.changed == 1 and want.counts() == [0, 3, 6]
    s.close()


def test_arena_grows_over_many_small_updates(ctx):
    rng = np.random.default_rng(22)
    leaves = [node() for _ in range(300)]
    nodes = [node(leaves)] + leaves
    s = Session(ctx, nodes)
    s.run([0])
    for i, f in enumerate(leaves):  # 300 calls of one node each
        f.done, f.value = True, fileset([(fid(rng), i)] * 2 + [(fid(rng), int(rng.integers(0, 99))) for _ in range(9)])
        s.push([1 + i])
        if i in (0, 92, 93, 94, 250):  # around the first growth (1024 rows) and beyond
            s.run([0])
    st, want = s.run([0])
    assert st.arena_rows == 3300 and st.nlive_est == 3300 and st.nlive == 3000
    s.close()


def test_set_values_device(ctx):
    """IDs hashed on the device and handed over without leaving it."""
    n_rows = 500
    msgs = [b"file %d" % i * (1 + i % 7) for i in range(n_rows)]
    offs = np.arange(n_rows, dtype=np.uint64) * 64
    lens = np.array([len(m) for m in msgs], dtype=np.uint64)
    arena = np.zeros(64 * n_rows, dtype=np.uint8)
    for o, m in zip(offs, msgs):
        arena[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
    sizes = lens.astype(np.int64)
    d_arena, d_ids, d_sizes = ctx.upload(arena), ctx.alloc(32 * n_rows), ctx.upload(sizes)
    plan = capi.ShaPlan(ctx, offs, lens)
    plan.run(d_arena.ptr, d_ids.ptr)
    counts = [0, 1, 64, 135, 300]
    leaves, at = [], 0
    for c in counts:
        leaves.append(node(rows=[(O.sha256(msgs[at + j]), int(sizes[at + j])) for j in range(c)]))
        at += c
    nodes = [node(leaves)] + leaves
    host = Session(ctx, nodes)
    _, want = host.run([0], [3])
    dev = capi.GcLiveset(ctx, *M.live_csr(nodes))
    dev.set_values_device([1, 2, 3, 4, 5], counts, d_ids.ptr, d_sizes.ptr)
    st = dev.run([0], [3])
    compare(dev, st, want)
    assert dev.filter().words().tobytes() == host.L.filter().words().tobytes()
    for o in (plan, dev, host):
        o.close()
    for b in (d_arena, d_ids, d_sizes):
        b.free()


# ---- the borrowed filter ---------------------------------------------------------------------
def test_borrowed_filter(ctx):
    rng = np.random.default_rng(31)
    live_rows = [(fid(rng), int(rng.integers(1, 1 << 30))) for _ in range(900)]
    nodes = [node([node(rows=live_rows[:400]), node(rows=live_rows[400:])])]
    nodes = M.all_nodes(nodes[0])
    s = Session(ctx, nodes)
    _, want = s.run([0])
    b = s.L.filter()
    wire = np.zeros(1 << 16, dtype=np.uint8)
    for marshal, fmt in ((b.marshal_binary, "rf_bloom_format_binary"), (b.marshal_json, "rf_bloom_format_json")):
        n = ctypes.c_uint64()
        capi._check(getattr(capi.lib(), fmt)(want.m, want.k, want.length, want.words.ctypes.data, len(want.words),
                                            wire.ctypes.data, len(wire), ctypes.byref(n)))
        assert marshal() == wire[:n.value].tobytes()
    # Repository.Collect in the run's stream: objects = the live files and as many others
    objs = np.frombuffer(b"".join(r[0] for r in live_rows) + rng.bytes(32 * 900), np.uint8).reshape(-1, 32)
    sizes = rng.integers(1, 1000, size=len(objs)).astype(np.int64)
    dead_want = np.flatnonzero(~want.contains(objs)).astype(np.uint64)
    assert 800 < len(dead_want) <= 900 and dead_want.min() >= 900
    other = capi.Context(0, host_threads=0)  # a caller's stream
    d_objs, d_sizes = ctx.upload(objs), ctx.upload(sizes)
    d_idx, d_n = ctx.alloc(8 * len(objs)), ctx.alloc(16)
    st = s.L.run([0], stream=other.stream)
    assert st.changed == 0
    s.L.filter().collect_device(d_objs.ptr, d_sizes.ptr, len(objs), d_idx.ptr, d_n.ptr, stream=other.stream)
    other.sync()
    n_dead, dead_bytes = d_n.to_numpy(np.uint64)[0], d_n.to_numpy(np.int64)[1]
    assert n_dead == len(dead_want) and dead_bytes == sizes[dead_want.astype(np.int64)].sum()
    assert d_idx.to_numpy(np.uint64)[:n_dead].tobytes() == dead_want.tobytes()
    assert s.L.filter().probe(objs).astype(bool).tolist() == want.contains(objs).tolist()
    other.close()
    # rf_bloom_destroy on the borrowed filter is a no-op: it still answers, and the next run reuses it
    capi.lib().rf_bloom_destroy(b._h)
    assert b.words().tobytes() == want.words.tobytes()
    b.close()  # the wrapper does not own it: this only drops the handle
    assert not b._h
    again = s.L.filter()
    assert again.words().tobytes() == want.words.tobytes()
    s.run([0])
    for d in (d_objs, d_sizes, d_idx, d_n):
        d.free()
    s.close()


# ---- refusals -------------------------------------------------------------------------------------
def test_refusals(ctx):
    nodes = [node([node(rows=[(bytes(32), 1)])])]
    nodes = M.all_nodes(nodes[0])
    L = capi.GcLiveset(ctx, *M.live_csr(nodes))
    with pytest.raises(capi.RfError) as e:
        L.filter()  # before any run
    assert e.value.code == capi.RF_EPRECONDITION
    bad = [lambda: L.run([2]), lambda: L.run([0], [2]), lambda: L.clear_values([5]),
           lambda: L.set_values([2], [0], np.zeros(0, np.uint8), np.zeros(0, np.int64))]
    for i, call in enumerate(bad):
        with pytest.raises(capi.RfError) as e:
            call()
        assert e.value.code == capi.RF_EINVAL and "out of range" in str(e.value), i
    with pytest.raises(capi.RfError) as e:
        capi.GcLiveset(ctx, np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32))
    assert e.value.code == capi.RF_EINVAL and "cycle" in str(e.value)
    # the object is still usable, and its filter belongs to its context: a plan of another refuses it
    L.set_values(*M.value_arrays(nodes))
    st = L.run([0])
    assert (st.nlive_est, st.nlive) == (1, 1)
    other = capi.Context(0, host_threads=0)
    plan = capi.EvalPlan(other, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint8),
                         np.zeros(2, np.uint64))
    assoc = capi.Assoc(other, 64)
    borrowed = L.filter()
    with pytest.raises(capi.RfError) as e:
        plan.run([0], assoc, 0, live=borrowed)
    assert e.value.code == capi.RF_EINVAL and "different contexts" in str(e.value)
    for o in (plan, assoc, other, L):
        o.close()
    assert not borrowed._h  # the filter died with its liveset: the wrapper no longer names it
    borrowed.close()


def test_row_bound(ctx):
    """More than RF_LIVE_MAX_ROWS rows in one run are refused after the offsets'
    scan, before any row array exists; the object goes on working."""
    rng = np.random.default_rng(41)
    big = node(rows=[(fid(rng), i) for i in range(70000)])
    leaf = node(rows=[(fid(rng), 1)] * 2)
    nodes = [node([leaf]), leaf, big]
    s = Session(ctx, nodes)
    st, _ = s.run([0], [2])
    times = capi.RF_LIVE_MAX_ROWS // 70000 + 1  # 15,340 entries of one writer: 2^30 < rows < 2^30 + 70,000
    bytes_before = st.device_bytes
    with pytest.raises(capi.RfError) as e:
        s.L.run([0], [2] * times)
    assert e.value.code == capi.RF_EINVAL and "rows in one run" in str(e.value)
    kept = s.L.stats()  # the previous run's figures and filter stand
    assert (kept.nlive_est, kept.nlive, kept.m, kept.k) == (st.nlive_est, st.nlive, st.m, st.k)
    assert kept.device_bytes < bytes_before + (1 << 20)  # no row arrays were made for the refused run
    assert s.L.filter().words().tobytes() == s.prev.words.tobytes()
    st2, _ = s.run([0], [2])
    assert st2.changed == 0
    s.close()
