"""Physical cache keys on the device (rf_physkeys_*, k13_physkeys.hip) against
the host form (rf_physkeys_flat) and the oracle (OFlow.physical_digest,
OFileset.material): seeded graphs and values, entry / node / graph-node counts
at the scan tiles' edges, materials at the gather tile's edges and at SHA-256's
padding edges, the value and graph shapes that can go wrong one by one, the
three update scopes, rows that must stay untouched, refusals that must change
nothing, and runs repeated byte for byte."""
import random

import numpy as np
import pytest

import physkeys_cases as PC
import reflow_oracle as O
from reflow_amd import capi

pytestmark = pytest.mark.gpu

T = capi.RF_PHYS_LIST_TILE
CT = capi.RF_PHYS_COPY_TILE
SELF, CONS = capi.RF_PHYS_SELF, capi.RF_PHYS_CONSUMERS


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


class Run:
    """A device object beside the oracle's flow nodes: set() gives values to
    both, update() runs the device and checks every row -- the affected ones
    against the oracle, all others against what they held before."""

    def __init__(self, ctx, nodes, seed=0):
        self.ctx, self.nodes = ctx, nodes
        self.g = PC.Graph(nodes, seed)
        for f in nodes:
            f.done = False
        self.pk = capi.PhysKeys(ctx, *self.g.open_args())
        self.rows = PC.pattern(self.g.n_rows)
        self.d_keys = ctx.upload(self.rows)

    def set(self, idx, vals, tree=False, d_ids32=None):
        if tree:
            self.pk.set_values(idx, sets=vals, d_ids32=d_ids32)
        else:
            f = capi.FilesetForest.from_host(self.ctx, [v.json() for v in vals])
            try:
                self.pk.set_values_forest(idx, f)
            finally:
                f.close()
        for i, v in zip(idx, vals):
            if i != capi.RF_PHYS_SKIP:
                self.nodes[i].done, self.nodes[i].value = True, v

    def clear(self, idx):
        self.pk.clear_values(idx)
        for i in idx:
            self.nodes[i].done = False

    def device_rows(self):
        return self.d_keys.to_numpy(np.uint8, 32 * self.g.n_rows).reshape(-1, 32)

    def update(self, listed, flags):
        o = self.pk.update(listed, flags, self.d_keys.ptr, self.g.n_rows, listed=True)
        aff = set(listed) if flags & SELF else set()
        if flags & CONS:
            aff |= set(self.g.consumers(listed))
        aff = sorted(i for i in aff if self.g.phys_row[i] != PC.NO_ROW)
        self.rows = self.g.want_rows(aff, self.rows)
        got = self.device_rows()
        assert (got == self.rows).all(), np.nonzero((got != self.rows).any(axis=1))[0][:8]
        comp = [self.nodes[i].physical_digest() is not None for i in aff]
        assert o.affected_nodes.tolist() == aff and o.computable_bits.tolist() == comp
        assert (o.affected, o.keys_written, o.keys_zeroed) == (len(aff), sum(comp), len(aff) - sum(comp))
        assert o.material_bytes == sum(len(self.nodes[i].physical_material()) for i, c in zip(aff, comp) if c)
        return o

    def check_values(self):
        idx, vals = PC.valued(self.nodes)
        for i, v in zip(idx, vals):
            assert self.pk.value_material(i) == v.material(), i
        assert self.pk.value_digests(idx) == [v.digest() for v in vals]
        assert self.pk.stats().n_values == len(idx)

    def close(self):
        self.pk.close()
        self.d_keys.free()


def fan(values, k_consumers=1, suffix="s"):
    """Valued sources and externs that each consume all of them in order."""
    src = [O.OFlow("OpMerge", value=v) for v in values]
    return src + [O.OFlow("OpExtern", list(src), url=suffix + str(j)) for j in range(k_consumers)]


# ---- seeded graphs ---------------------------------------------------------------
@pytest.mark.parametrize("seed,n", [(1, 1), (2, 9), (3, 150), (4, 700)])
def test_random_graphs(ctx, seed, n):
    nodes = PC.random_flows(seed, n)
    idx, vals = PC.valued(nodes)
    r = Run(ctx, nodes, seed)
    flat_keys, flat_mats = capi.physkeys_flat(*r.g.open_args(), idx, r.g.n_rows, sets=vals, keys=PC.pattern(r.g.n_rows))
    half = len(idx) // 2
    r.set(idx[:half], vals[:half])
    r.update(idx[:half], CONS)
    r.set(idx[half:], vals[half:], tree=True)
    r.update(idx[half:], CONS | SELF)
    r.update(list(range(n)), SELF)
    assert (r.device_rows() == flat_keys).all()
    assert [r.pk.value_material(i) for i in idx] == flat_mats
    r.check_values()
    r.close()


# ---- the scan tiles' edges ----------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_entries_per_value_at_tile_edges(ctx, count):
    """A Map of `count` entries beside a small one, and a List of `count` leaves
    (count + 1 forest nodes), so that entries and nodes cross the tiles."""
    rng = random.Random(count)
    big = PC.files(rng, count, plen=4 if count else 0)
    leaves = O.OFileset(list=[PC.files(rng, 1, plen=2) for _ in range(count)]) if count else O.OFileset()
    r = Run(ctx, fan([PC.files(rng, 2), big, leaves, PC.files(rng, 1)]))
    r.set([0, 1, 2, 3], [f.value for f in r.nodes[:4]])
    o = r.update([1], CONS)
    assert o.keys_written == 1
    r.check_values()
    r.close()


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_graph_nodes_at_tile_edges(ctx, n):
    """n graph nodes: one valued source, every other node its consumer -- each
    third without a key row -- so that the affected list, the per-affected scans
    and the segment table cross their tiles."""
    rng = random.Random(n)
    src = O.OFlow("OpMerge", value=PC.files(rng, 1))
    nodes = [src] + [O.OFlow("OpExtern" if j % 3 else "OpMerge", [src], url=str(j)) for j in range(1, n)]
    r = Run(ctx, nodes, n)
    r.update([0], CONS)  # no value yet: every affected row becomes zero
    r.set([0], [src.value])
    o = r.update([0], CONS)
    assert o.affected == o.keys_written == len(r.g.keyed) > n // 2
    r.close()


# ---- the gather tile's edges, SHA-256's padding edges ------------------------------
@pytest.mark.parametrize("total", [55, 56, 63, 64, 119, 120, CT - 1, CT, CT + 1, 2 * CT, 3 * CT + 5])
def test_material_lengths(ctx, total):
    """One consumer whose material is exactly `total` bytes, behind one whose
    material ends one byte before a 16-byte boundary; a suffix-only node of the
    same length."""
    rng = random.Random(total)
    a, b = PC.sized(rng, 47), PC.sized(rng, 34 + (total - 34) // 2)
    sa, sb = O.OFlow("OpMerge", value=a), O.OFlow("OpMerge", value=b)
    rest = total - len(b.material())
    nodes = [sa, sb, O.OFlow("OpExtern", [sa], url=""), O.OFlow("OpExtern", [sb], url="u" * rest),
             O.OFlow("OpExtern", [], url="v" * total), O.OFlow("OpExtern", [sa, sb, sa], url="w")]
    r = Run(ctx, nodes)
    r.set([0, 1], [a, b])
    assert len(nodes[3].physical_material()) == total == len(nodes[4].physical_material())
    o = r.update([0, 1, 4], CONS | SELF)
    assert o.keys_written == 4
    r.close()


def test_segments_across_tiles(ctx):
    """A dep's material that starts in one gather tile and ends two tiles later,
    a path longer than a tile, and empty materials between them."""
    rng = random.Random(5)
    vals = [PC.sized(rng, 1000), O.OFileset(), PC.files(rng, 200, plen=7), O.OFileset(map={"q" * (CT + 77): (PC.fid(rng), 1)}),
            O.OFileset(list=[O.OFileset(), O.OFileset()]), PC.sized(rng, 34)]
    assert len(vals[2].material()) > 2 * CT
    r = Run(ctx, fan(vals, 3))
    r.set(list(range(6)), vals)
    assert r.update([0], CONS).keys_written == 3
    r.check_values()
    r.close()


# ---- values and graphs, one shape each -----------------------------------------------
def test_value_shapes(ctx):
    """List of Lists; a node with both List and Map (the Map is ignored); an empty
    value; paths of length 0 and 1, with bytes >= 0x80, with an escape to decode."""
    A, B, C = (bytes([k]) * 32 for k in (1, 2, 3))
    leaf = O.OFileset(map={"": (A, 1), "b": (B, 2), "é\"\n\\<": (C, 3), "日": (A, 4)})
    vals = [O.OFileset(list=[O.OFileset(list=[leaf, O.OFileset()]), leaf]),
            O.OFileset(map={"ignored": (A, 1)}, list=[O.OFileset(map={"x": (B, 1)})]),
            O.OFileset()]
    for tree in (False, True):
        r = Run(ctx, fan(vals) + [O.OFlow("OpExec", [], image="", cmd="")])
        r.set([0, 1, 2], vals, tree=tree)
        r.update([0, 1, 2, 3, 4], SELF)
        assert r.pk.value_material(1) == b"x\x00\x05" + B and r.pk.value_material(2) == b""
        assert r.pk.value_digests([2]) == [O.sha256(b"")]
        assert r.device_rows()[r.g.phys_row[4]].tobytes() == O.sha256(b"")  # no deps, an empty suffix
        r.check_values()
        r.close()


def test_graph_shapes(ctx):
    """A dep listed twice, a 33-dep node, deps only partly valued, a value
    replaced and a value cleared."""
    rng = random.Random(8)
    src = [O.OFlow("OpMerge", value=PC.files(rng, rng.randint(0, 3))) for _ in range(33)]
    nodes = src + [O.OFlow("OpExec", src, image="i", cmd="c", argmap=[(True, 1), (False, 2)]),
                   O.OFlow("OpExtern", [src[0], src[0], src[1]], url="twice"),
                   O.OFlow("OpExtern", [src[2]], url="one")]
    r = Run(ctx, nodes)
    r.set(list(range(32)), [f.value for f in src[:32]])
    o = r.update(list(range(32)), CONS)
    assert (o.keys_written, o.keys_zeroed) == (2, 1)  # the 33-dep node waits for its last dep
    r.set([32], [src[32].value])
    assert r.update([32], CONS).keys_written == 1
    before = r.device_rows()[r.g.phys_row[34]].tobytes()
    st = r.pk.stats()
    r.set([0], [PC.files(rng, 5)])  # replaced: the new key, the old bytes stale
    assert r.update([0], CONS).keys_written == 2
    assert r.device_rows()[r.g.phys_row[34]].tobytes() != before
    st2 = r.pk.stats()
    assert st2.stale_bytes > st.stale_bytes or len(src[0].value.material()) == 0
    assert st2.arena_bytes > st.arena_bytes and st2.n_values == 33 and st2.device_bytes > st2.arena_bytes
    r.clear([0, 2])  # cleared: the consumers' rows go back to zero
    o = r.update([0, 2], CONS)
    assert (o.keys_written, o.keys_zeroed) == (0, 3)
    assert not r.device_rows()[[r.g.phys_row[i] for i in (33, 34, 35)]].any()
    assert r.pk.stats().n_values == 31
    with pytest.raises(capi.RfError):
        r.pk.value_material(0)
    r.close()


def test_scopes_and_untouched_rows(ctx):
    """SELF, CONSUMERS and both; a consumer reached from two listed nodes is
    affected once; every other row keeps the pattern it was filled with."""
    rng = random.Random(2)
    a, b = (O.OFlow("OpExtern", [], url=u, value=PC.files(rng, 2)) for u in "ab")
    c = O.OFlow("OpExec", [a, b], image="c", cmd="")
    d = O.OFlow("OpExec", [c], image="d", cmd="")
    e = O.OFlow("OpExtern", [b], url="e")
    r = Run(ctx, [a, b, c, d, e])
    r.set([0, 1], [a.value, b.value])
    assert r.update([0, 1], CONS).affected_nodes.tolist() == [2, 4]
    untouched = [r.g.phys_row[i] for i in (0, 1, 3)]
    assert (r.device_rows()[untouched] == PC.pattern(r.g.n_rows)[untouched]).all()
    assert r.update([0, 1], SELF).affected_nodes.tolist() == [0, 1]
    assert r.update([1, 2, 1], SELF | CONS).affected_nodes.tolist() == [1, 2, 3, 4]
    assert r.update([3], CONS).affected == 0
    spare = [x for x in range(r.g.n_rows) if x not in set(r.g.phys_row)]
    assert (r.device_rows()[spare] == PC.pattern(r.g.n_rows)[spare]).all()
    r.close()


def test_tree_values_with_device_ids(ctx):
    """Values given as a tree whose File IDs are device rows (K1's output)."""
    rng = random.Random(4)
    vals = [PC.random_value(rng) for _ in range(20)]
    b = capi.FilesetTreeBuilder()
    roots = [b.add(v) for v in vals]
    tree = b.struct()
    d_ids = ctx.upload(b._keep["ids"])
    tree.ids32 = None
    r = Run(ctx, fan(vals, 2))
    r.pk.set_values(list(range(20)), tree=tree, roots=roots, d_ids32=d_ids.ptr)
    for f in r.nodes[:20]:
        f.done = True
    assert r.update([0], CONS).keys_written == 2
    r.check_values()
    d_ids.free()
    r.close()


# ---- refusals -------------------------------------------------------------------------
def test_refusals_change_nothing(ctx):
    rng = random.Random(6)
    vals = [PC.files(rng, 2), PC.files(rng, 1)]
    r = Run(ctx, fan(vals, 2))
    r.set([0], vals[:1])
    r.update([0, 1], CONS)

    def refused(call):
        rows, stats = r.device_rows().tobytes(), r.pk.stats()
        with pytest.raises(capi.RfError) as e:
            call()
        assert e.value.code == capi.RF_EINVAL
        s = r.pk.stats()
        assert r.device_rows().tobytes() == rows
        assert (s.n_values, s.arena_bytes, s.stale_bytes) == (stats.n_values, stats.arena_bytes, stats.stale_bytes)
        assert r.pk.value_material(0) == vals[0].material()

    good = capi.FilesetForest.from_host(ctx, [v.json() for v in vals])
    mixed = capi.FilesetForest.from_host(ctx, [vals[1].json(), b'{"List":[]}'])
    host = capi.FilesetForest.flat([v.json() for v in vals])
    refused(lambda: r.pk.set_values_forest([1, 4], good))      # a node >= n
    refused(lambda: r.pk.set_values_forest([1, 0], mixed))     # a refused document with a real node
    refused(lambda: r.pk.set_values_forest([0, 1], host))      # a host-form forest
    refused(lambda: r.pk.update([4], SELF, r.d_keys.ptr, r.g.n_rows))
    refused(lambda: r.pk.update([0], 0, r.d_keys.ptr, r.g.n_rows))
    refused(lambda: r.pk.update([0], 4, r.d_keys.ptr, r.g.n_rows))
    refused(lambda: r.pk.update([0], CONS, r.d_keys.ptr, min(r.g.phys_row[2], r.g.phys_row[3])))  # a row >= n_rows
    refused(lambda: r.pk.clear_values([9]))
    refused(lambda: r.pk.value_digests([1]))                   # no value
    r.pk.set_values_forest([1, capi.RF_PHYS_SKIP], mixed)      # the refused document skipped: fine
    r.nodes[1].done, r.nodes[1].value = True, vals[1]
    assert r.update([1], CONS).keys_written == 2
    for f in (good, mixed, host):
        f.close()
    r.close()
    for kw in (dict(deps=[1]), dict(deps=[2]), dict(dep_ptr=[0, 1, 0]), dict(phys_row=[0, 0]),
               dict(suffix_ptr=[0, 2, 1])):
        a = dict(dict(dep_ptr=[0, 0, 1], deps=[0], phys_row=[PC.NO_ROW, 0], suffix_ptr=[0, 1, 2], suffix=np.zeros(2, np.uint8)), **kw)
        with pytest.raises(capi.RfError) as e:
            capi.PhysKeys(ctx, **a)
        assert e.value.code == capi.RF_EINVAL


def test_duplicate_nodes_keep_the_last_value(ctx):
    rng = random.Random(7)
    a, b = PC.files(rng, 3), PC.files(rng, 1)
    r = Run(ctx, fan([a]))
    r.set([0, capi.RF_PHYS_SKIP, 0], [a, a, b])
    assert r.pk.value_material(0) == b.material()
    assert r.update([0], CONS).keys_written == 1
    r.close()


# ---- the same bytes every time ---------------------------------------------------------
def test_same_bytes_every_time(ctx):
    nodes = PC.random_flows(12, 400)
    idx, vals = PC.valued(nodes)
    seen = []
    for _ in range(2):
        r = Run(ctx, nodes, 12)
        for f, v in zip([nodes[i] for i in idx], vals):
            f.value = v
        r.set(idx, vals)
        r.update(idx, CONS | SELF)
        seen.append((r.device_rows().tobytes(), [r.pk.value_material(i) for i in idx], r.pk.value_digests(idx)))
        r.close()
    assert seen[0] == seen[1]
