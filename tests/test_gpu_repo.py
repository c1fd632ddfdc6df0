"""The repository index on the device (rf_repo_*, k9_repo.hip) against its CPU
model (tests/repo_model.py: a dict plus per-group first-occurrence dedup):
every status, size, per-group count, list entry and statistic, exactly -- for
the index (chained batches, first wins, tombstones, growth), missing() in the
row form at the kernels' edge sizes, NeedTransfer over TestCacheLookup's flow,
random flows and hand-built shapes, Collect with the liveset's filter, and the
plan / missing / reject sequence."""
import ctypes
import random

import numpy as np
import pytest

import flowgen
import live_model as LM
import plan_model as PM
import reflow_oracle as O
import repo_model as M
from reflow_amd import capi

pytestmark = pytest.mark.gpu

TILE = capi.RF_REPO_LIST_TILE
POISON = 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


# ---- helpers ---------------------------------------------------------------------
def new_ids(rng, n):
    return [rng.bytes(32) for _ in range(n)]


def check_stats(repo, model):
    st, want = repo.stats(), model.stats()
    got = {k: getattr(st, k) for k in want}
    assert got == want
    assert st.device_bytes >= 44 * st.capacity


class Pair:
    """A device index and its model, written together."""

    def __init__(self, ctx, capacity=0):
        self.ctx, self.dev, self.ref = ctx, capi.Repo(ctx, capacity), M.Repo(capacity)

    def put(self, ids, sizes, device=False):
        want = self.ref.put(ids, sizes, device_form=device)
        if device:
            d_ids, d_sz = self.ctx.upload(M.ids_array(ids)), self.ctx.upload(np.array(sizes, np.int64))
            d_st = self.ctx.alloc(4 * max(len(ids), 1))
            d_st.fill(POISON)
            self.dev.put_device(d_ids.ptr, d_sz.ptr, len(ids), d_st.ptr)
            got = d_st.to_numpy(np.int32)[:len(ids)]
            for b in (d_ids, d_sz, d_st):
                b.free()
        else:
            got = self.dev.put(M.ids_array(ids), sizes)
        assert got.tolist() == want.tolist()
        return got

    def remove(self, ids, device=False):
        want = self.ref.remove(ids)
        if device:
            d_ids, d_out = self.ctx.upload(M.ids_array(ids)), self.ctx.alloc(max(len(ids), 1))
            d_out.fill(POISON)
            self.dev.remove_device(d_ids.ptr, len(ids), d_out.ptr)
            got = d_out.to_numpy(np.uint8)[:len(ids)]
            d_ids.free()
            d_out.free()
        else:
            got = self.dev.remove(M.ids_array(ids))
        assert got.tolist() == want.tolist()

    def stat(self, ids):
        want = self.ref.stat(ids)
        assert self.dev.stat(M.ids_array(ids)).tolist() == want.tolist()
        if not len(ids):
            return
        d_ids, d_out = self.ctx.upload(M.ids_array(ids)), self.ctx.alloc(8 * max(len(ids), 1))
        self.dev.stat_device(d_ids.ptr, len(ids), d_out.ptr)
        self.ctx.sync()
        assert d_out.to_numpy(np.int64)[:len(ids)].tolist() == want.tolist()
        d_ids.free()
        d_out.free()

    def close(self):
        self.dev.close()


def compare_missing(got, want, cap, row_form=True, listed=("miss_rows", "miss_ids32", "miss_sizes")):
    """Every array of one call against the model's; the list arrays are
    written below min(n_listed, cap) and keep their poison from there on."""
    for f in ("n_files", "n_missing", "missing_bytes", "miss_ptr"):
        if getattr(got, f) is not None:
            assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    if not row_form and got.status is not None:
        assert got.status.tobytes() == want.status.tobytes()
    if got.n_listed is not None:
        assert got.n_listed == want.n_listed
    w = min(want.n_listed, cap)
    for f in listed:
        a = getattr(got, f)
        if a is None or (f == "miss_rows" and not row_form):
            continue
        assert len(a) == cap
        assert a[:w].tobytes() == getattr(want, f)[:w].tobytes(), f
        assert a[w:].tobytes() == bytes([POISON]) * a[w:].nbytes, f


def run_missing(pair, groups, cap=None, **kw):
    counts, ids, sizes = M.flatten(groups)
    want = pair.ref.missing(groups)
    cap = len(sizes) if cap is None else cap
    got = pair.dev.missing(counts, ids, sizes, cap=cap, poison=POISON, **kw)
    compare_missing(got, want, cap)
    check_stats(pair.dev, pair.ref)
    return got, want


class DevOut:
    """Device arrays for an rf_repo_missing_out, poisoned; read() brings them back."""
    SHAPES = {"n_files": (np.uint32, "g"), "n_missing": (np.uint32, "g"), "missing_bytes": (np.int64, "g"),
              "status": (np.int32, "g"), "miss_ptr": (np.uint64, "g1"), "miss_rows": (np.uint64, "c"),
              "miss_ids32": (np.uint8, "c32"), "miss_sizes": (np.int64, "c"), "n_listed": (np.uint64, "one")}

    def __init__(self, ctx, n_groups, cap, fields):
        self.n = {"g": n_groups, "g1": n_groups + 1, "c": cap, "c32": 32 * cap, "one": 1}
        self.o, self.bufs = capi.RepoMissingOut(), {}
        self.o.cap = cap
        for f in fields:
            dt, k = self.SHAPES[f]
            b = ctx.alloc(max(self.n[k], 1) * np.dtype(dt).itemsize)
            b.fill(POISON)
            self.bufs[f] = b
            setattr(self.o, f, b.ptr)

    def read(self):
        res = capi.RepoMissing()
        for f, b in self.bufs.items():
            dt, k = self.SHAPES[f]
            setattr(res, f, b.to_numpy(dt)[:self.n[k]])
        if res.miss_ids32 is not None:
            res.miss_ids32 = res.miss_ids32.reshape(-1, 32)
        if res.n_listed is not None:
            res.n_listed = int(res.n_listed[0])
        return res

    def free(self):
        for b in self.bufs.values():
            b.free()


# ---- 1. the index ------------------------------------------------------------------
def test_chained_batches_host_and_device_forms(ctx):
    rng = np.random.default_rng(1)
    pool = new_ids(rng, 900)
    p = Pair(ctx)
    for step in range(8):
        device = step % 2 == 1
        pick = [pool[int(j)] for j in rng.integers(0, len(pool), size=int(rng.integers(1, 400)))]
        # an ID's size is a function of the ID, but for a few rows that state another
        sizes = [i[0] + 256 * i[1] + (1 if rng.random() < 0.05 else 0) for i in pick]
        p.put(pick, sizes, device=device)
        gone = [pool[int(j)] for j in rng.integers(0, len(pool), size=int(rng.integers(0, 120)))]
        p.remove(gone, device=device)
        p.stat(pool)
        check_stats(p.dev, p.ref)
    assert p.ref.stats()["tombstones"] > 0 and p.ref.stats()["objects"] > 100
    p.put([], [])
    p.remove([])
    p.stat([])
    p.close()


def test_one_id_twice_in_a_batch_first_wins(ctx):
    rng = np.random.default_rng(2)
    a, b, c, d = new_ids(rng, 4)
    for device in (False, True):
        p = Pair(ctx)
        got = p.put([a, b, a, a, b, c], [5, 1, 5, 6, 2, 0], device=device)  # equal and differing sizes
        assert got.tolist() == [0, 0, 0, capi.RF_EINTEGRITY, capi.RF_EINTEGRITY, 0]
        p.stat([a, b, c, d])
        # against the index: the later batch's first row of an ID is compared with the stored size
        got = p.put([a, a, d, d], [6, 5, 7, 7], device=device)
        assert got.tolist() == [capi.RF_EINTEGRITY, 0, 0, 0]
        p.stat([a, b, c, d])
        check_stats(p.dev, p.ref)
        # many copies of one ID, the lowest row carrying the size that stays
        e = new_ids(rng, 1)[0]
        sizes = [3] + [int(x) for x in rng.integers(2, 5, size=2999)]
        got = p.put([e] * 3000, sizes, device=device)
        assert got[0] == 0 and (got == capi.RF_EINTEGRITY).sum() == sum(s != 3 for s in sizes)
        p.stat([e])
        p.close()


def test_tombstoned_id_put_again_with_another_size(ctx):
    rng = np.random.default_rng(3)
    ids = new_ids(rng, 50)
    for device in (False, True):
        p = Pair(ctx)
        p.put(ids, list(range(50)), device=device)
        p.remove(ids[:20] + ids[:5], device=device)  # the second mention of an ID finds it gone
        assert p.ref.stats()["tombstones"] == 20
        p.stat(ids)
        p.put(ids[:10] + ids[:10], [100 + i for i in range(10)] + [7] * 10, device=device)  # fresh objects
        assert p.ref.stats()["tombstones"] == 10
        p.stat(ids)
        check_stats(p.dev, p.ref)
        p.close()


def test_negative_sizes(ctx):
    rng = np.random.default_rng(4)
    a, b, c = new_ids(rng, 3)
    p = Pair(ctx)
    p.put([a], [1])
    with pytest.raises(capi.RfError) as e:  # the host form: the whole batch, nothing changes
        p.dev.put(M.ids_array([b, c]), [2, -3])
    assert e.value.code == capi.RF_EINVAL and p.ref.put([b, c], [2, -3]) is None
    p.stat([a, b, c])
    check_stats(p.dev, p.ref)
    got = p.put([c, b, c, c, a], [-1, 2, 4, 5, -9], device=True)  # the device form: that row alone
    assert got.tolist() == [capi.RF_EINVAL, 0, 0, capi.RF_EINTEGRITY, capi.RF_EINVAL]
    p.stat([a, b, c])
    check_stats(p.dev, p.ref)
    p.close()


@pytest.mark.parametrize("device", [False, True])
def test_growth_in_one_batch_and_in_many(ctx, device):
    rng = np.random.default_rng(5)
    ids = new_ids(rng, 6000)
    sizes = [i[3] for i in ids]
    # one batch far past the growth point of the smallest table
    p = Pair(ctx)
    assert p.dev.stats().capacity == capi.RF_REPO_MIN_SLOTS
    p.put(ids[:512], sizes[:512], device=device)
    assert p.dev.stats().rebuilds == 0  # exactly half the slots
    p.remove(ids[:40], device=device)
    before = p.dev.stat(M.ids_array(ids)).tolist()
    p.put(ids[512:513], sizes[512:513], device=device)  # live + tombstones + 1 pass half: rebuilt
    st = p.dev.stats()
    assert (st.capacity, st.rebuilds, st.tombstones) == (2048, 1, 0)
    after = p.dev.stat(M.ids_array(ids)).tolist()
    assert after[:512] == before[:512] and after[513:] == before[513:] and after[512] == sizes[512]
    p.put(ids[513:] + ids[:40], sizes[513:] + sizes[:40], device=device)
    assert p.dev.stats().capacity == 16384 and p.dev.stats().rebuilds == 2
    p.stat(ids)
    check_stats(p.dev, p.ref)
    p.close()
    # many small batches with removals in between
    p = Pair(ctx)
    for lo in range(0, 3000, 150):
        p.put(ids[lo:lo + 150], sizes[lo:lo + 150], device=device)
        p.remove(ids[lo:lo + 150:7], device=device)
    assert p.dev.stats().rebuilds >= 2
    p.stat(ids[:3200])
    check_stats(p.dev, p.ref)
    p.close()


# ---- 2. missing, the row form --------------------------------------------------------
@pytest.fixture(scope="module")
def world(ctx):
    """4000 files, each with one size; every second one is in the repository."""
    rng = np.random.default_rng(6)
    ids = new_ids(rng, 4000)
    files = [(i, int(i[5]) + 1) for i in ids]
    p = Pair(ctx)
    p.put(ids[::2], [f[1] for f in files[::2]])
    yield p, files
    p.close()


def pick_rows(rng, files, n, span=None):
    span = len(files) if span is None else span
    return [files[int(j)] for j in rng.integers(0, span, size=n)]


def test_no_groups_and_empty_groups(ctx, world):
    p, files = world
    rng = np.random.default_rng(7)
    got, want = run_missing(p, [])
    assert got.miss_ptr.tolist() == [0] and got.n_listed == 0
    run_missing(p, [[], [], []])
    # groups of no rows at the start, in the middle and at the end
    got, want = run_missing(p, [[], [], pick_rows(rng, files, 5), [], [], pick_rows(rng, files, 70), []])
    assert want.n_listed > 0 and want.n_files[3] == 0


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_one_group_at_the_tile_edges(ctx, world, n):
    p, files = world
    rng = np.random.default_rng(n)
    got, want = run_missing(p, [pick_rows(rng, files, n, span=max(n // 2, 1))])  # repeats inside the group
    assert want.n_files[0] <= n and (n == 1 or want.n_files[0] < n)
    first = (got.miss_rows.tobytes(), got.miss_ids32.tobytes(), got.n_missing.tobytes(), got.missing_bytes.tobytes())
    again, _ = run_missing(p, [pick_rows(np.random.default_rng(n), files, n, span=max(n // 2, 1))])
    assert first == (again.miss_rows.tobytes(), again.miss_ids32.tobytes(), again.n_missing.tobytes(),
                     again.missing_bytes.tobytes())  # two runs give equal bytes


def test_a_group_that_straddles_a_list_tile_and_many_small_groups(ctx, world):
    p, files = world
    rng = np.random.default_rng(8)
    absent = [f for f in files[1::2]]
    # 1000 rows, then a group of absent files across the tile boundary at row 1024, then the rest
    got, want = run_missing(p, [pick_rows(rng, files, 1000), absent[:60], pick_rows(rng, files, 1100)])
    assert want.n_missing[1] == 60 and want.miss_ptr[1] < TILE < want.rows[int(want.miss_ptr[2]) - 1]
    # 3,000 groups of 0-3 rows
    groups = [pick_rows(rng, files, int(rng.integers(0, 4))) for _ in range(3000)]
    got, want = run_missing(p, groups)
    assert want.n_listed > 1000 and got.miss_ptr[-1] == want.n_listed


def test_equal_rows_two_sizes_two_groups_all_and_nothing(ctx, world):
    p, files = world
    present, absent = files[0], files[1]
    got, want = run_missing(p, [[absent] * 2500])  # all rows equal
    assert (want.n_files.tolist(), want.n_missing.tolist(), want.rows) == ([1], [1], [0])
    run_missing(p, [[present] * 2500])
    # one ID with two sizes: two files, and both are missing or neither
    got, want = run_missing(p, [[(absent[0], 1), (absent[0], 2), (absent[0], 1)],
                                [(present[0], 9), (present[0], present[1])]])
    assert want.n_files.tolist() == [2, 2] and want.n_missing.tolist() == [2, 0] and want.missing_bytes.tolist() == [3, 0]
    # one file in two groups is counted in both
    got, want = run_missing(p, [[absent, present], [present, absent], [absent]])
    assert want.n_missing.tolist() == [1, 1, 1] and want.rows == [0, 3, 4]
    rng = np.random.default_rng(9)
    everything = [[files[int(j)] for j in rng.integers(0, 2000, size=300) * 2] for _ in range(4)]
    got, want = run_missing(p, everything)
    assert want.n_listed == 0 and want.n_files.sum() > 0
    nothing = [[files[int(j)] for j in rng.integers(0, 2000, size=300) * 2 + 1] for _ in range(4)]
    got, want = run_missing(p, nothing)
    assert want.n_listed == want.n_files.sum() > 0


def test_caps(ctx, world):
    p, files = world
    rng = np.random.default_rng(10)
    groups = [pick_rows(rng, files, 40) for _ in range(30)]
    counts, ids, sizes = M.flatten(groups)
    want = p.ref.missing(groups)
    n = want.n_listed
    assert n > 100
    exact = p.dev.missing(counts, ids, sizes, cap=n, poison=POISON)
    compare_missing(exact, want, n)
    for cap in (0, n - 1):  # nothing at or beyond cap is written, n_listed is still set
        short = p.dev.missing(counts, ids, sizes, cap=cap, poison=POISON, check=False)
        assert short.rc == capi.RF_EINVAL and short.n_listed == n
        compare_missing(short, want, cap)
    # without list arrays nothing has to fit
    counted = p.dev.missing(counts, ids, sizes, cap=0, want=("n_missing", "n_listed", "miss_ptr"), poison=POISON)
    compare_missing(counted, want, 0)
    # the device form: ranks below cap are written, the caller compares
    d_ct, d_ids, d_sz = ctx.upload(counts), ctx.upload(ids), ctx.upload(sizes)
    for cap in (0, 7, n):
        out = DevOut(ctx, len(groups), cap, capi.RepoMissing.FIELDS)
        p.dev.missing_device(d_ct.ptr, len(groups), d_ids.ptr, d_sz.ptr, len(sizes), out.o)
        ctx.sync()
        got = out.read()
        got.status = None
        compare_missing(got, want, cap)
        out.free()
    check_stats(p.dev, p.ref)
    # fewer rows given than the counts sum to: refused, the object stays usable
    out = DevOut(ctx, len(groups), 0, ("n_listed",))
    with pytest.raises(capi.RfError) as e:
        p.dev.missing_device(d_ct.ptr, len(groups), d_ids.ptr, d_sz.ptr, len(sizes) - 1, out.o)
    assert e.value.code == capi.RF_EINVAL
    out.free()
    run_missing(p, groups)
    for b in (d_ct, d_ids, d_sz):
        b.free()


@pytest.mark.parametrize("seed", range(6))
def test_any_subset_of_output_pointers(ctx, world, seed):
    p, files = world
    rng = np.random.default_rng(100 + seed)
    groups = [pick_rows(rng, files, int(rng.integers(0, 30))) for _ in range(50)]
    fields = [f for f in capi.RepoMissing.FIELDS if f != "status"]
    subset = [f for f in fields if rng.random() < 0.5] if seed else []
    counts, ids, sizes = M.flatten(groups)
    want = p.ref.missing(groups)
    got = p.dev.missing(counts, ids, sizes, want=subset, poison=POISON)
    assert [f for f in fields if getattr(got, f) is not None] == subset
    compare_missing(got, want, len(sizes))
    out = DevOut(ctx, len(groups), len(sizes), subset)
    d_ct, d_ids, d_sz = ctx.upload(counts), ctx.upload(ids), ctx.upload(sizes)
    p.dev.missing_device(d_ct.ptr, len(groups), d_ids.ptr, d_sz.ptr, len(sizes), out.o)
    ctx.sync()
    compare_missing(out.read(), want, len(sizes))
    check_stats(p.dev, p.ref)
    for b in (d_ct, d_ids, d_sz):
        b.free()
    out.free()


def test_row_limit_leaves_the_object_usable(ctx, world):
    p, files = world
    counts = np.full(5, 1 << 28, np.uint32)  # 2^30 + 2^28 rows stated: refused before anything is read
    rc = capi.lib().rf_repo_missing(p.dev._h, counts.ctypes.data, 5, counts.ctypes.data, counts.ctypes.data,
                                    ctypes.byref(capi.RepoMissingOut()))
    assert rc == capi.RF_EINVAL and b"2^30" in capi.lib().rf_last_error()
    run_missing(p, [files[:10]])


# ---- 3. need_transfer ------------------------------------------------------------------
class Flow:
    """A liveset over OFlow nodes with its values, and the model's view of them."""

    def __init__(self, ctx, nodes, device_values=False):
        self.ctx, self.nodes = ctx, nodes
        self.edge_ptr, self.edges = LM.live_csr(nodes)
        self.L = capi.GcLiveset(ctx, self.edge_ptr, self.edges)
        self.values = {}
        self.push(range(len(nodes)), device_values)

    def push(self, which, device=False):
        nd, ct, ids, sz = LM.value_arrays(self.nodes, [int(i) for i in which])
        if not len(nd):
            return
        if device:
            d_ids, d_sz = self.ctx.upload(ids if len(ids) else np.zeros(32, np.uint8)), \
                self.ctx.upload(sz if len(sz) else np.zeros(1, np.int64))
            self.L.set_values_device(nd, ct, d_ids.ptr, d_sz.ptr)
            d_ids.free()
            d_sz.free()
        else:
            self.L.set_values(nd, ct, ids, sz)
        for i in nd.tolist():
            self.values[i] = LM.value_rows(self.nodes[i].value)

    def all_files(self):
        return sorted({r for rows in self.values.values() for r in rows})

    def close(self):
        self.L.close()


def run_need_transfer(p, fl, nodes):
    want = p.ref.need_transfer(fl.edge_ptr, fl.edges, fl.values, nodes)
    cap = want.n_rows
    got = p.dev.need_transfer(fl.L, nodes, cap=cap, poison=POISON)
    compare_missing(got, want, cap, row_form=False)
    check_stats(p.dev, p.ref)
    # the device form
    d_nodes = p.ctx.upload(np.array(list(nodes) or [0], np.uint32))
    out = DevOut(p.ctx, len(nodes), cap, [f for f in capi.RepoMissing.FIELDS if f != "miss_rows"])
    p.dev.need_transfer_device(fl.L, d_nodes.ptr, len(nodes), out.o)
    p.ctx.sync()
    compare_missing(out.read(), want, cap, row_form=False)
    out.free()
    d_nodes.free()
    return got, want


def test_cache_lookup_flow_with_the_intern_done(ctx):
    """TestCacheLookup's flow (test/evaltest/eval_test.go:174-230): the intern's
    value is set, what reads it is ready; a node above a dep without a value is
    refused alone."""
    nodes, ix = PM.cache_lookup_flow()  # (every MapFlow is among the nodes)
    intern = nodes[ix["intern"]]
    intern.done, intern.value = True, LM.files("a:a", "b:b", "c:c")
    val = nodes[ix["mapexec"]].deps[0]  # the exec's argument: an OpVal holding the empty Fileset
    val.done = True
    fl = Flow(ctx, nodes)
    p = Pair(ctx)
    rows = LM.value_rows(intern.value)
    p.put([rows[0][0], rows[2][0]], [1, 1])  # b is not in the repository
    ready = [ix["groupby"], ix["mapexec"]]
    got, want = run_need_transfer(p, fl, ready + [ix["extern"]])
    assert want.status.tolist() == [0, 0, capi.RF_EPRECONDITION]
    assert want.n_files.tolist() == [3, 0, 0] and want.n_missing.tolist() == [1, 0, 0]
    assert want.missing_bytes.tolist() == [1, 0, 0] and want.ids == [O.sha256(b"b")]
    fl.close()
    p.close()


@pytest.mark.parametrize("seed,n,device_values", [(1, 60, False), (2, 150, True), (3, 300, False)])
def test_random_flows(ctx, seed, n, device_values):
    root, _ = flowgen.random_dag(seed, n)
    nodes = LM.all_nodes(root)
    fl = Flow(ctx, nodes, device_values)
    rng = random.Random(seed)
    files = fl.all_files()
    assert len(files) > 20
    p = Pair(ctx)
    present = rng.sample(files, len(files) // 2)
    p.put([f[0] for f in present], [f[1] for f in present])
    every = list(range(len(nodes)))
    got, want = run_need_transfer(p, fl, every)
    assert (want.status == capi.RF_EPRECONDITION).sum() > 0 and want.n_listed > 0
    run_need_transfer(p, fl, [rng.randrange(len(nodes)) for _ in range(40)])  # any order, nodes listed twice
    run_need_transfer(p, fl, [])
    fl.close()
    p.close()


def test_hand_built_shapes(ctx):
    rng = np.random.default_rng(11)

    def leaf(rows):
        return O.OFlow("OpIntern", done=True, value=O.OFileset(map={"p%d" % i: r for i, r in enumerate(rows)}))
    f = [(i, int(i[0])) for i in new_ids(rng, 3000)]
    a, b, c = leaf(f[:3]), leaf(f[2:5]), leaf([])
    big = leaf(f[5:2905])
    pending = O.OFlow("OpIntern")
    twice = O.OFlow("OpExec", [a, b, a, a])          # a dep listed twice: its rows repeat, the dedup removes them
    bad = O.OFlow("OpExec", [a, pending, b])         # a dep without a value
    none = O.OFlow("OpExec", [])                     # no edges
    empty = O.OFlow("OpExec", [c, c])                # values of no rows
    wide = O.OFlow("OpExec", [big, a, big])          # rows beyond a list tile, repeated
    nodes = LM.all_nodes(O.OFlow("OpMerge", [twice, bad, none, empty, wide]))
    ix = {id(x): i for i, x in enumerate(nodes)}
    fl = Flow(ctx, nodes)
    p = Pair(ctx)
    p.put([x[0] for x in f[::3]], [x[1] for x in f[::3]])
    order = [ix[id(x)] for x in (twice, bad, none, empty, wide, bad, twice)]
    got, want = run_need_transfer(p, fl, order)
    assert want.status.tolist() == [0, capi.RF_EPRECONDITION, 0, 0, 0, capi.RF_EPRECONDITION, 0]
    assert want.n_files.tolist() == [5, 0, 0, 0, 2903, 0, 5]  # the bad group's neighbours are unaffected
    # a value replaced between two calls
    a.value = O.OFileset(map={"q": f[2999], "r": f[0]})
    fl.push([ix[id(a)]])
    got, want = run_need_transfer(p, fl, order)
    assert want.n_files.tolist() == [5, 0, 0, 0, 2902, 0, 5]
    pending.done, pending.value = True, O.OFileset(map={"only": f[2998]})
    fl.push([ix[id(pending)]])
    got, want = run_need_transfer(p, fl, order)
    assert want.status.tolist() == [0] * 7 and want.n_files[1] == 6
    # a node out of range: the host form refuses the call
    with pytest.raises(capi.RfError) as e:
        p.dev.need_transfer(fl.L, [0, len(nodes)], cap=0)
    assert e.value.code == capi.RF_EINVAL
    # another context's liveset
    other = capi.Context(0, host_threads=0)
    L2 = capi.GcLiveset(other, *LM.live_csr(nodes))
    with pytest.raises(capi.RfError) as e:
        p.dev.need_transfer(L2, [0], cap=0)
    assert e.value.code == capi.RF_EINVAL
    L2.close()
    other.close()
    fl.close()
    p.close()


class Tables:
    def __init__(self, ctx):
        self.dev, self.ref = capi.Assoc(ctx, 1024), O.InmemoryAssoc()

    def put(self, kind, keys, vals):
        st = self.dev.put(kind, np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(vals), np.uint8))
        assert (st == capi.RF_OK).all()
        for k, v in zip(keys, vals):
            self.ref.put(kind, None, k, v)


def plan_case(ctx):
    """Three layers of execs over interns with values; every second exec of the
    top layers and some interns are cached.  (nodes, keys, roots, tables, plan)"""
    rng = np.random.default_rng(12)
    files = [(i, int(i[1]) + 1) for i in new_ids(rng, 400)]
    interns = [O.OFlow("OpIntern", url="u%d" % i) for i in range(60)]
    mid = [O.OFlow("OpExec", [interns[int(j)] for j in rng.integers(0, 60, size=3)], image="i", cmd="m%d" % i)
           for i in range(80)]
    top = [O.OFlow("OpExec", [mid[int(j)] for j in rng.integers(0, 80, size=2)], image="i", cmd="t%d" % i)
           for i in range(40)]
    nodes = top + mid + interns
    for i, f in enumerate(interns):
        if i % 3:  # two thirds of the interns are done, with a value
            f.done = True
            f.value = O.OFileset(map={"p%d" % k: files[int(j)] for k, j in enumerate(rng.integers(0, 400, size=5))})
    keys = [[PM.fileset_id(1000 + i)] for i in range(len(nodes))]
    t = Tables(ctx)
    cached = [i for i in range(len(nodes)) if not nodes[i].done and i % 2 == 0]
    t.put(0, [keys[i][0] for i in cached], [PM.fileset_id(i) for i in cached])
    dep_ptr, deps = PM.flow_csr(nodes)
    key_ptr, key_rows = PM.key_arrays(keys)
    plan = capi.EvalPlan(ctx, dep_ptr, deps, PM.flow_flags(nodes), key_ptr)
    return nodes, keys, key_rows, list(range(len(top))), t, plan, files


def test_ready_list_fed_device_to_device(ctx):
    nodes, keys, key_rows, roots, t, plan, files = plan_case(ctx)
    plan.run(roots, t.dev, 0, keys=key_rows)
    want_plan = PM.plan(nodes, roots, t.ref, 0, node_keys=keys)
    ready = want_plan.list(PM.READY)[0]
    assert len(ready) > 5
    fl = Flow(ctx, nodes)
    p = Pair(ctx)
    p.put([f[0] for f in files[::2]], [f[1] for f in files[::2]])
    d_nodes, d_found = ctx.alloc(4 * len(nodes)), ctx.alloc(8)
    plan.list_device(PM.READY, len(nodes), d_nodes.ptr, None, None, None, d_found.ptr)
    ctx.sync()
    assert d_found.to_numpy(np.uint64)[0] == len(ready)
    want = p.ref.need_transfer(fl.edge_ptr, fl.edges, fl.values, ready.tolist())
    assert (want.status == 0).sum() > 0
    out = DevOut(ctx, len(ready), want.n_rows, [f for f in capi.RepoMissing.FIELDS if f != "miss_rows"])
    p.dev.need_transfer_device(fl.L, d_nodes.ptr, len(ready), out.o)
    ctx.sync()
    compare_missing(out.read(), want, want.n_rows, row_form=False)
    check_stats(p.dev, p.ref)
    for b in (d_nodes, d_found):
        b.free()
    out.free()
    fl.close()
    p.close()
    plan.close()
    t.dev.close()


# ---- 4. collect ----------------------------------------------------------------------------
def test_collect_with_the_borrowed_filter(ctx):
    """TestGC: after the root is done Collect removes exactly `unrooted`; then a
    larger repository against the oracle's bloom."""
    nodes, ix = LM.gc_flow()
    LM.gc_stage(nodes, ix, 3)
    fl = Flow(ctx, nodes)
    fl.L.run([ix["pullup"]])
    want_live = LM.live(nodes, [ix["pullup"]])
    ids, sizes = LM.gc_objects()
    rng = np.random.default_rng(13)
    extra = new_ids(rng, 5000)  # dead but for the filter's false positives
    all_ids = [bytes(i) for i in ids] + extra
    all_sizes = sizes.tolist() + [int(i[2]) for i in extra]
    p = Pair(ctx)
    p.put(all_ids, all_sizes)
    b = fl.L.filter()
    dead_idx, dead_bytes = b.collect(M.ids_array(all_ids), np.array(all_sizes, np.int64))  # rf_bloom_collect
    contains = dict(zip(all_ids, want_live.contains(all_ids)))
    want = p.ref.collect(lambda i: contains[i])
    got = p.dev.collect(b)
    assert got == want == (len(dead_idx), dead_bytes)
    assert 4990 < got[0] <= 5001 and p.ref.stat([bytes(ids[7])]).tolist() == [-1]
    p.stat(all_ids)
    check_stats(p.dev, p.ref)
    assert p.dev.collect(b) == (0, 0)  # nothing more to remove
    # a nil liveset removes everything
    want = p.ref.collect(None)
    assert p.dev.collect(None) == want and want[0] == 7 + (5000 - (got[0] - 1))
    p.stat(all_ids[:50])
    check_stats(p.dev, p.ref)
    assert p.dev.stats().objects == 0
    fl.close()
    p.close()


def test_collect_with_a_loaded_filter_whose_length_grew(ctx):
    """A plain rf_bloom loaded with a bitset shorter than m, then grown by
    rf_bloom_add (the length lives on the device): Collect keeps everything the
    filter contains, as rf_bloom_collect and the oracle's bloom say."""
    rng = np.random.default_rng(15)
    m, k, length = 1 << 15, 4, 1000
    need = (length + 63) // 64
    words = np.zeros((m + 63) // 64, dtype=np.uint64)
    words[:need] = rng.integers(0, 2 ** 63, size=need, dtype=np.uint64)
    b = capi.Bloom.load(ctx, m, k, words, length)
    ids = new_ids(rng, 3000)
    sizes = [int(i[4]) + 1 for i in ids]
    live = ids[:1500]
    b.add(M.ids_array(live))
    want_words, ln = words.copy(), np.array([length], dtype=np.uint64)
    O.lib().orc_bloomlive_add_batch(want_words.ctypes.data, ln.ctypes.data, m, k, b"".join(live), len(live))
    assert length < int(ln[0]) == b.params()[2]
    inside = np.zeros(len(ids), dtype=np.uint8)
    O.lib().orc_bloomlive_contains_batch(want_words.ctypes.data, int(ln[0]), m, k, b"".join(ids), len(ids),
                                         inside.ctypes.data, 1)
    assert inside[:1500].all() and not inside[1500:].all()
    contains = dict(zip(ids, inside.astype(bool).tolist()))
    p = Pair(ctx)
    p.put(ids, sizes)
    dead_idx, dead_bytes = b.collect(M.ids_array(ids), np.array(sizes, np.int64))  # rf_bloom_collect
    want = p.ref.collect(lambda i: contains[i])
    got = p.dev.collect(b)
    assert got == want == (len(dead_idx), dead_bytes) and 0 < got[0] <= 1500
    p.stat(ids)
    assert (p.dev.stat(M.ids_array(live)) >= 0).all()  # nothing the filter contains was removed
    check_stats(p.dev, p.ref)
    b.close()
    p.close()


# ---- 5. plan, missing over the hits' values, reject --------------------------------------------
def test_plan_missing_reject(ctx):
    nodes, keys, key_rows, roots, t, plan, files = plan_case(ctx)
    plan.run(roots, t.dev, 0, keys=key_rows)
    want_plan = PM.plan(nodes, roots, t.ref, 0, node_keys=keys)
    hits = [int(i) for i in want_plan.list(PM.HIT)[0]]
    assert plan.list(PM.HIT)[0].tolist() == hits and len(hits) > 10
    # the cached values of the hits, as the caller unmarshals them: a few files each
    rng = np.random.default_rng(14)
    values = [[files[int(j)] for j in rng.integers(0, 400, size=int(rng.integers(0, 6)))] for _ in hits]
    p = Pair(ctx)
    p.put([f[0] for f in files[:300]], [f[1] for f in files[:300]])  # the last hundred files are gone
    got, want = run_missing(p, values)
    failing = [h for h, m in zip(hits, got.n_missing.tolist()) if m]
    assert 0 < len(failing) < len(hits)
    plan.reject(failing, t.dev, 0, keys=key_rows)
    want_r = PM.reject(nodes, roots, t.ref, 0, failing, node_keys=keys)
    assert plan.states().tolist() == want_r.states.tolist()
    fresh = capi.EvalPlan(ctx, *PM.flow_csr(nodes), PM.flow_flags(nodes, invalid=failing), PM.key_arrays(keys)[0])
    fresh.run(roots, t.dev, 0, keys=key_rows)  # a fresh run with RF_PLAN_F_INVALID on them
    assert fresh.states().tobytes() == plan.states().tobytes()
    for state in range(5):
        assert fresh.list(state)[0].tobytes() == plan.list(state)[0].tobytes()
    fresh.close()
    plan.close()
    p.close()
    t.dev.close()
