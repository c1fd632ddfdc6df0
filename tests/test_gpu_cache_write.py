"""The cache write on the device (rf_eval_wave_cache_write, k11_cwrite.hip,
cache_write.cpp) against its CPU model (tests/cwrite_model.py: Eval.CacheWrite,
eval.go:1113-1154): the reference's TestCacheWrite flow, seeded random flows
evaluated bottom-up with the values marshalled, hashed and written on the
device -- after every batch the assoc's and the index's scans against the
model's dicts, the counters and the per-node bytes --, the refusals, the
round trip through a fresh wave object, and a batch that makes both tables
grow."""
import numpy as np
import pytest

import cwrite_model as M
import plan_model as P
import reflow_oracle as O
import wave_model as W
from lowering import Lowered
from reflow_amd import capi

pytestmark = pytest.mark.gpu

KIND = M.KIND


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def assoc_dict(a, kind=KIND):
    keys, vals, _ = a.scan(kind)
    return {k.tobytes(): v.tobytes() for k, v in zip(keys, vals)}


def repo_dict(r):
    ids, sizes, n, _ = r.scan()
    return {i.tobytes(): int(s) for i, s in zip(ids[:n], sizes[:n])}


class KeyGraph:
    """The key rows as the input slots of a loaded graph, in a shuffled slot
    order (key_slots is the indirection), beside one job that hashes slot 0."""

    def __init__(self, ctx, n_keys, seed):
        low = Lowered()
        slots = [low.new_slot() for _ in range(max(n_keys, 1))]
        low.jobs.append((low.new_slot(), bytearray(32), [(0, slots[0])]))
        self.g = capi.Graph.from_arrays(ctx, low.arrays())
        self.key_slots = np.random.default_rng(seed).permutation(n_keys).astype(np.uint32)
        self.first = True

    def set(self, flat):
        """flat [K, 32]: row r goes to slot key_slots[r]."""
        if len(flat):
            self.g.set_slots(self.key_slots, np.ascontiguousarray(flat, np.uint8).reshape(-1))
        self.g.recompute(full=self.first)
        self.first = False


class Both(M.ModelTarget):
    """play()'s calls on the device objects and on the model; check() compares."""

    def __init__(self, ctx, case, form, with_repo=True):
        super().__init__(case)
        self.ctx, self.form = ctx, form
        self.assoc = capi.Assoc(ctx, 64)
        self.repo = capi.Repo(ctx, 0) if with_repo else None
        dep_ptr, deps = P.flow_csr(case.nodes)
        key_ptr, flat = P.key_arrays(case.keys())
        self.kg = KeyGraph(ctx, len(flat), 5) if form == "graph" else None
        self.w = capi.EvalWave(ctx, dep_ptr, deps, self.model.flags, key_ptr,
                               self.kg.key_slots if self.kg else None)
        self.d_keys = None

    def _keys(self, keys):
        """The device-side key arguments of begin / step / cache_write."""
        flat = P.key_arrays(keys)[1]
        if self.kg:
            self.kg.set(flat)
            return dict(graph=self.kg.g)
        if self.d_keys is not None:
            self.d_keys.free()
        self.d_keys = self.ctx.upload(flat.reshape(-1) if len(flat) else np.zeros(32, np.uint8))
        return dict(d_keys=self.d_keys.ptr)

    def begin(self, roots, keys, no_cache_extern):
        super().begin(roots, keys, no_cache_extern)
        self.w.begin(roots, self.assoc, KIND, no_cache_extern=no_cache_extern, **self._keys(keys))

    def step(self, finished, keys):
        super().step(finished, keys)
        self.w.step(finished, self.assoc, KIND, **self._keys(keys))

    def write(self, listed, values, keys, no_cache_extern):
        want = super().write(listed, values, keys, no_cache_extern)
        # marshal -> digests -> write, nothing of it through the host
        batch = capi.JsonBatch(self.ctx, values)
        d_fsids = self.ctx.alloc(32 * max(len(values), 1))
        batch.digests_device(d_fsids.ptr)
        o, per = self.w.cache_write(listed, d_fsids.ptr, batch.device()[2], self.assoc, KIND, repo=self.repo,
                                    no_cache_extern=no_cache_extern, **self._keys(keys))
        written, puts, skipped, per_want = want
        assert (o.nodes_written, o.keys_put) == (written, puts)
        assert [o.skipped_not_cacheable, o.skipped_extern, o.skipped_no_key] == skipped
        assert per.tolist() == per_want
        batch.close()
        d_fsids.free()

    def check(self):
        assert self.w.states().tolist() == self.model.states.tolist()
        assert assoc_dict(self.assoc) == self.tables.assoc_entries()
        if self.repo is not None:
            assert repo_dict(self.repo) == self.tables.repo

    def close(self):
        self.w.close()
        self.assoc.close()
        if self.repo is not None:
            self.repo.close()
        if self.kg:
            self.kg.g.close()
        if self.d_keys is not None:
            self.d_keys.free()


# ---- 1. the reference's cache-write flow ---------------------------------------------------
def test_cache_write_flow(ctx):
    """TestCacheWrite (test/evaltest/eval_test.go:129-172): exec(intern).  After
    the write every CacheKey of the exec maps to the fsid, the fsid is SHA-256
    of the oracle's JSON of the value, and the repository holds (fsid, len)."""
    intern = O.OFlow("OpIntern", url="internurl")
    ex = O.OFlow("OpExec", [intern], image="image", cmd="command")
    nodes = [ex, intern]
    case = M.C.FlowCase(nodes, [0], [])
    t = Both(ctx, case, "keys")
    t.begin([0], case.keys(), False)
    t.check()
    for i, value in ((1, W.files("a/b/c", "a/b/d", "x/y/z")), (0, W.files("execout"))):
        assert int(t.model.states[i]) == W.READY
        nodes[i].done, nodes[i].value = True, value
        keys = case.keys()
        t.step([i], keys)
        t.write([i], [value], keys, False)
        t.check()
        fsid = O.sha256(value.json())
        present = [k for k in keys[i] if k != W.ZERO]
        assert present == nodes[i].cache_keys() and len(present) == (2 if i == 0 else 1)
        got = t.assoc.get(KIND, np.frombuffer(b"".join(present), np.uint8))
        assert all(v.tobytes() == fsid for v in got[0]) and got[1].all()
        assert t.repo.stat(np.frombuffer(fsid, np.uint8)).tolist() == [len(value.json())]
    t.close()


# ---- 2. random flows -------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["keys", "graph"])
@pytest.mark.parametrize("seed,n,nce", M.SEEDS)
def test_random_flows(ctx, seed, n, nce, form):
    """What these cover is asserted on the model alone by tests/test_cwrite_model.py."""
    case = M.CwCase(seed, n)
    nodes = case.nodes
    done0 = [f.done for f in nodes]
    t = Both(ctx, case, form)
    seen = M.play(case, t, no_cache_extern=nce)
    assert seen["batches"] >= 3 and all(t.model.states[r] == W.DONE for r in case.roots)
    # The round trip: evaluated again by a fresh wave object over the same graph,
    # every node a write served is a HIT when its turn comes, under its first
    # present key and with the fsid the tables hold for it.
    written = {i for i in seen["ran"] if M.participation(int(t.model.flags[i]), [b"k"], nce)[0] == M.WRITTEN
               and i not in case.no_key and i not in case.invalid}
    for f, d in zip(nodes, done0):
        f.done = d
    dep_ptr, deps = P.flow_csr(nodes)
    keys = case.keys()
    w = capi.EvalWave(ctx, dep_ptr, deps, P.flow_flags(nodes, case.invalid), P.key_arrays(keys)[0])
    w.begin(case.roots, t.assoc, KIND, keys=P.key_arrays(keys)[1])
    entries, served = t.tables.assoc_entries(), set()
    while True:
        hit_nodes, which, vals, _ = w.list(W.HIT, W.LAST)
        ready = [int(i) for i in w.list(W.READY, W.LAST)[0]]
        assert not written & set(ready)
        for i, j, v in zip(hit_nodes.tolist(), which.tolist(), vals):
            first = next(q for q, k in enumerate(keys[i]) if k != W.ZERO)
            if i in written:
                assert j == first and v.tobytes() == entries[keys[i][first]], i
                served.add(i)
        done = hit_nodes.tolist() + ready
        if not done:
            break
        for i in done:
            nodes[i].done = True
        keys = case.keys()
        w.step(done, t.assoc, KIND, keys=P.key_arrays(keys)[1])
    assert served == written and len(written) >= 3
    w.close()
    t.close()


def test_without_a_repository(ctx):
    case = M.CwCase(1, 80)
    t = Both(ctx, case, "keys", with_repo=False)
    t.tables.write = lambda *a, _w=t.tables.write, **k: _w(*a, **dict(k, repo=False))
    M.play(case, t)
    assert t.tables.repo == {} and len(t.tables.assoc) > 0
    t.close()


# ---- 3. refusals -----------------------------------------------------------------------------
def test_refusals(ctx):
    flags = np.array([W.F_CACHEABLE] * 3, np.uint8)
    ptr = np.array([0, 1, 1, 1], np.uint64)  # 0 -> 1
    deps = np.array([1], np.uint32)
    key_ptr = np.array([0, 1, 2, 3], np.uint64)
    keys = np.frombuffer(b"".join(O.sha256(b"k%d" % i) for i in range(3)), np.uint8)
    kg = KeyGraph(ctx, 3, 1)
    w = capi.EvalWave(ctx, ptr, deps, flags, key_ptr, kg.key_slots)
    a, other = capi.Assoc(ctx, 64), capi.Context(0, host_threads=0)
    foreign_assoc, foreign_repo = capi.Assoc(other, 64), capi.Repo(other, 0)
    repo = capi.Repo(ctx, 0)
    d_keys = ctx.upload(keys)
    d_f = ctx.upload(np.frombuffer(P.fileset_id(1) + P.fileset_id(0), np.uint8))
    d_s = ctx.upload(np.array([5, 6], np.int64))
    a.put(KIND, keys[64:], np.frombuffer(P.fileset_id(2), np.uint8))

    def refused(code, nodes=(1,), assoc=a, rp=repo, **kw):
        before = (assoc_dict(a), repo_dict(repo))
        with pytest.raises(capi.RfError) as e:
            w.cache_write(list(nodes), d_f.ptr, d_s.ptr, assoc, KIND, repo=rp, **(kw or dict(d_keys=d_keys.ptr)))
        assert e.value.code == code, str(e.value)
        assert (assoc_dict(a), repo_dict(repo)) == before

    refused(capi.RF_EPRECONDITION)                       # before any begin
    w.begin([0], a, KIND, d_keys=d_keys.ptr)
    assert w.states().tolist() == [W.TODO, W.READY, W.UNSEEN]
    refused(capi.RF_EINVAL)                              # READY, not DONE
    w.step([1], a, KIND, d_keys=d_keys.ptr)
    refused(capi.RF_EINVAL, nodes=(1, 0))                # one of two is not DONE
    refused(capi.RF_EINVAL, nodes=(1, 2))                # never reached
    refused(capi.RF_EINVAL, nodes=(3,))                  # out of range
    refused(capi.RF_EINVAL, assoc=foreign_assoc)         # mixed contexts
    refused(capi.RF_EINVAL, rp=foreign_repo)
    kg.set(keys.reshape(-1, 32))
    kg.g.set_slots([kg.key_slots[0]], np.frombuffer(O.sha256(b"moved"), np.uint8))  # a pending change on g
    refused(capi.RF_EPRECONDITION, graph=kg.g)
    kg.g.set_slots([kg.key_slots[0]], keys[:32])
    kg.g.recompute()
    o, per = w.cache_write([1], d_f.ptr, d_s.ptr, a, KIND, graph=kg.g, repo=repo)
    assert (o.nodes_written, o.keys_put, per.tolist()) == (1, 1, [1])
    assert assoc_dict(a) == {keys[32:64].tobytes(): P.fileset_id(1), keys[64:].tobytes(): P.fileset_id(2)}
    assert repo_dict(repo) == {P.fileset_id(1): 5}
    o, per = w.cache_write([], None, None, a, KIND, d_keys=d_keys.ptr)  # an empty list is valid
    assert (o.nodes_written, o.keys_put) == (0, 0)
    for x in (d_keys, d_f, d_s):
        x.free()
    for x in (w, a, repo, foreign_assoc, foreign_repo, kg.g, other):
        x.close()


# ---- 4. table growth ---------------------------------------------------------------------------
def test_growth_and_rewrite(ctx):
    """One batch large enough to make the assoc and the index grow; a second
    batch rewrites the same keys with new fsids: no key count changes, every
    value is the new fsid, and the old fsid objects stay in the index."""
    n = capi.RF_REPO_MIN_SLOTS + 300  # > half of the smallest tables' slots, more than one tile
    flags = np.full(n, W.F_CACHEABLE | W.F_DONE, np.uint8)
    ptr = np.zeros(n + 1, np.uint64)
    key_ptr = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    keys = np.frombuffer(b"".join(O.sha256(b"grow %d" % i) for i in range(2 * n)), np.uint8).reshape(-1, 32)
    w = capi.EvalWave(ctx, ptr, np.zeros(0, np.uint32), flags, key_ptr)
    a, repo = capi.Assoc(ctx, 16), capi.Repo(ctx, 0)
    d_keys = ctx.upload(keys.reshape(-1))
    w.begin(list(range(n)), a, KIND, d_keys=d_keys.ptr)
    assert w.stats().counts[W.DONE] == n
    cap0, slots0 = a.stats()[1], repo.stats().capacity
    nodes = np.arange(n, dtype=np.uint32)
    model = M.Tables()
    for gen in range(2):
        fsids = [O.sha256(b"fsid %d %d" % (gen, i)) for i in range(n)]
        sizes = [100 * gen + i for i in range(n)]
        d_f = ctx.upload(np.frombuffer(b"".join(fsids), np.uint8))
        d_s = ctx.upload(np.array(sizes, np.int64))
        o, per = w.cache_write(nodes, d_f.ptr, d_s.ptr, a, KIND, d_keys=d_keys.ptr, repo=repo)
        want = model.write(flags, [W.DONE] * n, [[keys[2 * i].tobytes(), keys[2 * i + 1].tobytes()] for i in range(n)],
                           nodes.tolist(), fsids, sizes)
        assert (o.nodes_written, o.keys_put, per.tolist()) == (want[0], want[1], want[3]) == (n, 2 * n, [2] * n)
        assert assoc_dict(a) == model.assoc_entries() and a.count(KIND) == (2 * n, 0)
        assert repo_dict(repo) == model.repo and repo.stats().objects == (gen + 1) * n
        if gen == 0:
            assert a.stats()[1] > cap0 and repo.stats().capacity > slots0 and repo.stats().rebuilds >= 1
        d_f.free()
        d_s.free()
    assert set(assoc_dict(a).values()) == {O.sha256(b"fsid 1 %d" % i) for i in range(n)}
    for x in (w, a, repo):
        x.close()
