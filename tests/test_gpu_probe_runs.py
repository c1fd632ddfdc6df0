"""The open-addressing tables' probe loops, entered on purpose: keys built
(tests/hashkeys.py) to share one 32-bit hash share their home slot in every
table, whatever its mask, so they form one probe run; with the hash
0xFFFFFFFE the home is mask - 1 and the run wraps round the table's end.

Covered, each bit-exact against the plain model the suite already has (first
occurrence, a dict, repo_model, live_model, plan_model): the K5 digest dedup,
the HBM assoc (Put / Get / delete / CAS / scan / growth / compact / save and
restore / lookup), the repository index (Put / Remove / Stat / tombstones /
Collect / rebuild), the two row-dedup tables with sizes (rf_repo_missing,
rf_repo_need_transfer, rf_liveset_run), and the plan's and the feed's inline
assoc_find.  No table here is ever more than half full.

The first test ties the host mirror of the hash to the device's: without it
every other test here could pass on a mirror that is wrong."""
import numpy as np
import pytest

import hashkeys as HK
import live_model as LM
import plan_model as PM
import reflow_oracle as O
import repo_model as RM
from reflow_amd import capi
from reflow_amd.workloads import Dag1000
from test_gpu_feed import Tracked
from test_gpu_liveset_walk import Session, node
from test_gpu_plan import Tables, hand_graph, run_and_compare
from test_gpu_repo import POISON, DevOut, Flow, Pair, check_stats, compare_missing, run_missing, run_need_transfer

pytestmark = pytest.mark.gpu

H = HK.WRAP_HASH
ZERO = bytes(32)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def rows_of(a):
    return [r.tobytes() for r in np.asarray(a, dtype=np.uint8).reshape(-1, 32)]


def nonzero_vals(rng, n):
    return rng.integers(1, 256, size=(n, 32), dtype=np.uint8)


def first_occurrence(d):
    first = {}
    return np.array([first.setdefault(r, i) for i, r in enumerate(rows_of(d))], dtype=np.uint32)


# ---- the mirror is the device's hash -----------------------------------------------------
def test_scan_order_is_the_mirrors_slot_order(ctx):
    """64 keys whose homes, by the mirror, are 16 slots apart in a table of 1024
    slots: no two collide, each sits in its home, and rf_assoc_scan lists in
    ascending slot order -- so the scan equals the keys sorted by hash & 1023
    iff the device hashes as the mirror does."""
    rng = np.random.default_rng(10)
    hashes = (rng.integers(0, 1 << 22, size=64, dtype=np.uint64) << np.uint64(10)) | (16 * np.arange(64, dtype=np.uint64) + 5)
    keys = HK.keys_with_hash(rng, hashes, 64)
    vals = nonzero_vals(rng, 64)
    order = rng.permutation(64)
    a = capi.Assoc(ctx, 512)  # (capacity in keys: 1024 slots)
    assert (a.put(0, keys[order], vals[order]) == 0).all()
    assert a.stats() == (64, 1024)
    k, v, kd = a.scan(-1)
    by_slot = np.argsort(HK.key_hash(keys) & np.uint32(1023), kind="stable")
    assert by_slot.tolist() == list(range(64))  # (as built: homes ascending)
    assert k.tobytes() == keys.tobytes() and v.tobytes() == vals.tobytes() and (kd == 0).all()
    a.close()


# ---- dedup -----------------------------------------------------------------------------
def test_dedup_one_wrapping_run_host_and_device_forms(ctx):
    """300 distinct keys of hash 0xFFFFFFFE (more than a block of 256: lanes of
    several waves and blocks race in one run, which wraps in whatever table
    dedup_table_slots picks), each three times, shuffled among 1000 random keys."""
    rng = np.random.default_rng(11)
    run = HK.keys_with_hash(rng, H, 300)
    d = np.concatenate([run, run, run, rng.integers(0, 256, size=(1000, 32), dtype=np.uint8)])
    d = d[rng.permutation(len(d))]
    want = first_occurrence(d)
    assert len(np.unique(want)) == 1300
    canon, nu = ctx.dedup_digests(d)
    assert canon.tolist() == want.tolist() and nu == 1300
    dd, dc, dn = ctx.upload(d), ctx.alloc(4 * len(d)), ctx.alloc(64)
    for _ in range(2):  # (the second call finds the context's table used)
        dc.fill(POISON)
        ctx.dedup_digests_device(dd.ptr, len(d), dc.ptr, dn.ptr)
        ctx.sync()
        assert dc.to_numpy(np.uint32).tolist() == want.tolist()
        assert int(dn.to_numpy(np.uint32, count=1)[0]) == 1300
    for b in (dd, dc, dn):
        b.free()


# ---- assoc -----------------------------------------------------------------------------
class AssocModel:
    """(kind, key) -> value; a zero value is a deleted key that keeps its slot."""

    def __init__(self):
        self.v = {}

    def put(self, kind, keys, vals, expect=None):
        out = []
        for i, (k, v) in enumerate(zip(rows_of(keys), rows_of(vals))):
            cur = self.v.setdefault((kind, k), ZERO)  # (a failed compare-and-set still claims the slot)
            e = ZERO if expect is None else rows_of(expect)[i]
            if e != ZERO and cur != e:
                out.append(capi.RF_EPRECONDITION)
                continue
            self.v[(kind, k)] = v
            out.append(capi.RF_OK)
        return out

    def get(self, kind, keys):
        vals = [self.v.get((kind, k), ZERO) for k in rows_of(keys)]
        return vals, [int(v != ZERO) for v in vals]

    def live(self, kind=None):
        return {(kd, k, v) for (kd, k), v in self.v.items() if v != ZERO and kind in (None, kd)}


def scan_set(a, kind=-1):
    k, v, kd = a.scan(kind)
    rows = list(zip(kd.tolist(), rows_of(k), rows_of(v)))
    assert len(set(rows)) == len(rows)
    return rows


KA, KB, KNONE = 0, 7, 3


def test_assoc_run_of_two_kinds(ctx, tmp_path):
    rng = np.random.default_rng(12)
    a, m = capi.Assoc(ctx, 512), AssocModel()  # (capacity in keys: 1024 slots)
    run = HK.keys_with_hash(rng, H, 100)
    absent = HK.keys_with_hash(rng, H, 50)

    def put(kind, keys, vals, expect=None):
        got = a.put(kind, keys, vals, expect)
        assert got.tolist() == m.put(kind, keys, vals, expect)
        return got

    def check_gets(t=None):
        t = a if t is None else t
        probe = np.concatenate([run, absent])
        for kind in (KA, KB, KNONE):
            vals, found = t.get(kind, probe)
            wv, wf = m.get(kind, probe)
            assert found.tolist() == wf and rows_of(vals) == wv, kind

    # one run of 150 entries over three batches: later batches probe past ready entries of
    # earlier launches and busy slots of their own; 50 key byte strings sit under both kinds
    put(KA, run[:30], nonzero_vals(rng, 30))
    put(KB, run[10:60], nonzero_vals(rng, 50))
    put(KA, run[30:], nonzero_vals(rng, 70))
    assert a.stats() == (150, 1024)
    check_gets()  # (the 50 absent keys of the same hash walk the whole run and end on the empty slot)
    # delete every third key
    put(KA, run[::3], np.zeros((len(run[::3]), 32), np.uint8))
    put(KB, run[10:60:3], np.zeros((len(run[10:60:3]), 32), np.uint8))
    check_gets()
    # compare-and-set on keys of the last batch (the run's far end): matching and stale expects,
    # on live keys, on a deleted key (90 = 3 * 30) and on a key that is not there
    far = run[88:100]
    cur, _ = a.get(KA, far)
    exp = cur.copy()
    exp[1::2] = nonzero_vals(rng, len(exp[1::2]))  # every second expect is stale
    exp[2] = 0xFF  # run[90] is deleted: any nonzero expect fails
    got = put(KA, far, nonzero_vals(rng, len(far)), exp)
    assert got.tolist() == [capi.RF_OK if i % 2 == 0 and i != 2 else capi.RF_EPRECONDITION for i in range(len(far))]
    stranger = HK.keys_with_hash(rng, H, 1)
    assert put(KA, stranger, nonzero_vals(rng, 1), nonzero_vals(rng, 1)).tolist() == [capi.RF_EPRECONDITION]
    assert a.stats() == (151, 1024)
    check_gets()
    # the deleted keys come back
    put(KA, run[::3], nonzero_vals(rng, len(run[::3])))
    check_gets()
    # a second run (another hash, home slot 0x345), one key per batch: inside it the scan order is
    # the insertion order; in the raced run only the set is fixed
    run2 = HK.keys_with_hash(rng, 0x5A5A5345, 20)
    for i in range(20):
        put((KA, KB)[i % 2], run2[i:i + 1], nonzero_vals(rng, 1))
    assert a.stats() == (171, 1024)
    rows = scan_set(a)
    assert set(rows) == m.live()
    in2 = {r.tobytes() for r in run2}
    assert [(kd, k) for kd, k, _ in rows if k in in2] == [((KA, KB)[i % 2], run2[i].tobytes()) for i in range(20)]
    in1 = {r.tobytes() for r in run} | {stranger.tobytes()}
    assert rows[0][1] in in1 and rows[-1][1] in in1  # the wrap: slots 0 and 1023 hold run keys
    assert all(k in in1 or k in in2 for _, k, _ in rows)
    for kind in (KA, KB):
        assert set(scan_set(a, kind)) == m.live(kind)
    # growth, twice: assoc_reserve rebuilds, and the rehash re-forms both runs; deleted keys keep a slot
    for n in (400, 700):
        cap = a.stats()[1]
        put(KA, rng.integers(0, 256, size=(n, 32), dtype=np.uint8), nonzero_vals(rng, n))
        assert a.stats()[1] > cap
    assert a.stats()[0] == len(m.v) == 171 + 1100
    check_gets()
    assert set(scan_set(a)) == m.live()
    # rf_assoc_lookup over nodes of 0..3 keys from the run (live, deleted, other kind only, absent)
    pool = np.concatenate([run, absent[:20]])
    counts = rng.integers(0, 4, size=120)
    key_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    lk = pool[rng.integers(0, len(pool), size=int(key_ptr[-1]))]
    for kind in (KA, KB):
        which, vals, kf, kv = a.lookup(kind, lk, key_ptr)
        wv, wf = m.get(kind, lk)
        assert kf.tolist() == wf and rows_of(kv) == wv
        for i in range(120):
            b, e = int(key_ptr[i]), int(key_ptr[i + 1])
            w = next((j - b for j in range(b, e) if wf[j]), -1)
            assert which[i] == w and vals[i].tobytes() == (wv[b + w] if w >= 0 else ZERO), (kind, i)
        assert (which == 0).sum() > 10 and (which == -1).sum() > 10 and (which > 0).sum() > 0
    # compaction drops the deleted keys
    live = len(m.live())
    assert live < len(m.v)
    a.compact()
    assert a.stats()[0] == live and a.count() == (live, 0)
    m.v = {k: v for k, v in m.v.items() if v != ZERO}
    check_gets()
    # save / restore: k5_assoc_load re-forms the runs
    path = str(tmp_path / "runs.assoc")
    a.save(path)
    b = capi.Assoc.restore(ctx, path)
    check_gets(b)
    assert set(scan_set(b)) == m.live() and b.stats()[0] == live
    b.close()
    a.close()


# ---- the repository index ----------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host_forms", "device_forms"])
def test_repo_index_run_with_tombstones(ctx, device):
    rng = np.random.default_rng(13)
    p = Pair(ctx)
    run = rows_of(HK.keys_with_hash(rng, H, 150))
    absent = rows_of(HK.keys_with_hash(rng, H, 40))
    sizes = {i: 1000 + j for j, i in enumerate(run)}

    def step():
        p.stat(run + absent)  # (absent IDs of the same hash walk the whole run)
        check_stats(p.dev, p.ref)

    p.put(run[:80], [sizes[i] for i in run[:80]], device=device)
    step()
    p.put(run[80:], [sizes[i] for i in run[80:]], device=device)
    step()
    gone = run[::3]
    p.remove(gone + gone[:5], device=device)  # tombstones give -1; everything behind one is still found
    assert p.ref.stats()["tombstones"] == 50
    step()
    # removed IDs put again with another size are fresh objects: the tombstone count goes down
    got = p.put(gone[:25], [7 + sizes[i] for i in gone[:25]], device=device)
    assert (got == capi.RF_OK).all() and p.ref.stats()["tombstones"] == 25
    step()
    # new colliding IDs while tombstones lie in the run
    more = rows_of(HK.keys_with_hash(rng, H, 30))
    p.put(more, list(range(30)), device=device)
    step()
    # one colliding ID twice in a batch with two sizes: the first wins
    x, y = rows_of(HK.keys_with_hash(rng, H, 2))
    got = p.put([x, y, x, run[1], x], [5, 6, 7, 1 + sizes[run[1]], 5], device=device)
    assert got.tolist() == [0, 0, capi.RF_EINTEGRITY, capi.RF_EINTEGRITY, 0]
    run += more + [x, y]
    step()
    # Collect against a filter that holds half of the run
    half = run[::2]
    live = PM.Liveset(half)
    b = capi.Bloom.load(ctx, live.m, live.k, live.words, live.length)
    want = p.ref.collect(live.contains)
    assert p.dev.collect(b) == want and 40 < want[0] < 100
    b.close()
    step()
    # random Puts force a rebuild: the tombstones go and the run is formed again
    before = p.ref.stats()
    assert before["tombstones"] > 60
    n = before["capacity"] // 2
    p.put([rng.bytes(32) for _ in range(n)], list(range(n)), device=device)
    after = p.ref.stats()
    assert after["rebuilds"] == before["rebuilds"] + 1 and after["tombstones"] == 0
    step()
    p.put(gone[25:], [sizes[i] for i in gone[25:]], device=device)  # (no tombstone to revive now: plain inserts)
    step()
    p.close()


# ---- row dedup with sizes ------------------------------------------------------------------
# Groups 2, 3 and 5 hold the run; 0 is a few plain rows, 1 and 4 are empty.  (The ord enters the
# row hash through an odd multiply, a bijection: the same (ID, size) can never have ONE hash in two
# groups.  hash_for_two_ords gives the next best: hashes with the same low 12 bits, so one home
# slot in every table of up to 4096 slots -- these tables have 1024 -- and it exists for these
# pairs of ordinals, not for (0, 1) or (1, 2).)
RUN_GROUPS = (2, 3, 5)
LOW = H & 0xFFF


@pytest.fixture(scope="module")
def row_groups():
    rng = np.random.default_rng(14)
    groups = [[(rng.bytes(32), int(rng.integers(0, 100))) for _ in range(5)] * 2, [], [], [], [], []]
    distinct = {g: [] for g in RUN_GROUPS}
    for g in RUN_GROUPS:  # different IDs of one row hash, and the same ID with two sizes
        sizes = rng.integers(1, 1 << 20, size=30).astype(np.int64)
        ids = HK.rows_with_hash(rng, H, g, sizes)
        base = list(zip(rows_of(ids), sizes.tolist()))
        twins = [(i, HK.size_twin(s)) for i, s in base[:6]]
        assert (HK.row_hash(g, RM.ids_array([i for i, _ in twins]), [s for _, s in twins]) == H).all()
        distinct[g] += base + twins
    for ga, gb in ((2, 3), (2, 5), (3, 5)):  # the same (ID, size) in two groups: two classes
        ha, hb = HK.hash_for_two_ords(ga, gb, LOW)
        sizes = rng.integers(1, 1 << 20, size=6).astype(np.int64)
        ids = HK.rows_with_hash(rng, ha, ga, sizes)
        assert (HK.row_hash(gb, ids, sizes) == hb).all() and ha & 0xFFF == hb & 0xFFF == LOW
        both = list(zip(rows_of(ids), sizes.tolist()))
        distinct[ga] += both
        distinct[gb] += both
    for g in RUN_GROUPS:  # each row twice, in any order
        rows = distinct[g] * 2
        groups[g] = [rows[j] for j in rng.permutation(len(rows))]
    n = sum(len(g) for g in groups)
    assert 280 <= n <= 320 and capi.RF_REPO_MIN_SLOTS == 1024  # (the row table: 1024 slots)
    return groups, distinct


def test_missing_rows_of_one_home_slot(ctx, row_groups):
    groups, distinct = row_groups
    p = Pair(ctx)
    every = sorted({i for g in RUN_GROUPS for i, _ in distinct[g]})
    p.put(every[::2], [1] * len(every[::2]))  # half of the IDs exist (by ID alone, whatever the size)
    got, want = run_missing(p, groups)
    assert want.n_files.tolist() == [5, 0, 48, 48, 0, 48]
    assert 0 < want.n_missing[2] < 48 and want.n_listed == int(want.n_missing.sum())
    # the device form
    counts, ids, sizes = RM.flatten(groups)
    d = [ctx.upload(x) for x in (counts, ids, sizes)]
    out = DevOut(ctx, len(groups), len(sizes), [f for f in capi.RepoMissing.FIELDS if f != "status"])
    p.dev.missing_device(d[0].ptr, len(groups), d[1].ptr, d[2].ptr, len(sizes), out.o)
    ctx.sync()
    compare_missing(out.read(), want, len(sizes))
    check_stats(p.dev, p.ref)
    out.free()
    for b in d:
        b.free()
    p.close()


def test_need_transfer_rows_of_one_home_slot(ctx, row_groups):
    """k9_nt_segments numbers a segment by the index of its node in `nodes`, and
    k9_locate gives a row its segment's number: a row's ordinal is its group's
    index in the call, as in the row form -- so the same rows, as the values of
    one dep per listed node, form the same run."""
    groups, distinct = row_groups
    leaves = [O.OFlow("OpIntern", done=True, value=O.OFileset(map={"p%04d" % i: r for i, r in enumerate(rows)}))
              for rows in groups]
    execs = [O.OFlow("OpExec", [leaf]) for leaf in leaves]
    nodes = LM.all_nodes(O.OFlow("OpMerge", execs))
    ix = {id(f): i for i, f in enumerate(nodes)}
    fl = Flow(ctx, nodes)
    p = Pair(ctx)
    every = sorted({i for g in RUN_GROUPS for i, _ in distinct[g]})
    p.put(every[1::2], [1] * len(every[1::2]))
    got, want = run_need_transfer(p, fl, [ix[id(e)] for e in execs])
    assert want.status.tolist() == [0] * 6 and want.n_files.tolist() == [5, 0, 48, 48, 0, 48]
    assert 0 < want.n_missing[5] < 48
    fl.close()
    p.close()


def test_liveset_rows_of_one_live_hash(ctx):
    """One root that is done: one value, so its ordinal is 0; about 300 rows of
    one live_hash with duplicates and equal-ID / other-size pairs."""
    rng = np.random.default_rng(15)
    sizes = rng.integers(1, 1 << 20, size=110).astype(np.int64)
    ids = HK.rows_with_hash(rng, H, 0, sizes)
    base = list(zip(rows_of(ids), sizes.tolist()))
    twins = [(i, HK.size_twin(s)) for i, s in base[:30]]
    rows = (base + twins) * 2 + base[:20]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    assert len(rows) == 300
    assert (HK.row_hash(0, RM.ids_array([i for i, _ in rows]), [s for _, s in rows]) == H).all()
    s = Session(ctx, [node(rows=rows)])
    st, want = s.run([0])
    assert (want.nlive_est, want.nlive) == (300, 140) and want.livebytes == sum(sz for _, sz in base + twins)
    s.close()


# ---- the plan and the feed through a run -----------------------------------------------------
def test_plan_lookups_through_a_run(ctx):
    """k7_plan's inline assoc_find: every key row is a key of the run -- half
    under the plan's kind, some under another kind only, the rest absent."""
    rng = np.random.default_rng(16)
    n = 127
    deps = [[j for j in (2 * i + 1, 2 * i + 2) if j < n] for i in range(n)]
    cacheable = [i % 5 != 0 for i in range(n)]  # (the root and every fifth node are merges)
    nodes = hand_graph(deps, cacheable)
    run = rows_of(HK.keys_with_hash(rng, H, 220))
    node_keys, at = [], 0
    for i in range(n):
        k = (1 + i % 2) if cacheable[i] else 0
        node_keys.append(run[at:at + k])
        at += k
    used = run[:at]
    t = Tables(ctx)
    present = [k for j, k in enumerate(used) if j % 4 < 2]
    other = [k for j, k in enumerate(used) if j % 4 >= 1 and j % 4 < 3]  # (j % 4 == 2: the other kind only)
    t.put(0, present, [PM.fileset_id(j) for j in range(len(present))])
    t.put(7, other, [PM.fileset_id(1000 + j) for j in range(len(other))])
    assert t.dev.stats()[0] == len(present) + len(other) <= 512
    for roots in ([0], list(range(0, n, 3))):
        p, want = run_and_compare(ctx, nodes, node_keys, roots, t)
        if len(roots) > 1:
            c = want.counts()
            assert c[PM.HIT] > 10 and c[PM.TODO] + c[PM.READY] > 10
            assert any(w == 1 for w, _, _ in want.hits.values())  # (a first key absent or of the other kind)
        p.close()
    t.close()


def test_feed_lookup_at_the_end_of_runs(ctx):
    """k6_feed's fused lookup: the changed slots' real cache keys each sit at
    the end of a run of three crafted keys of the real key's own hash, put
    first.  feed_lookup_device agrees with a host Get of the same keys and with
    the dict."""
    dag = Dag1000(22, 32)
    a = dag.arrays()
    t = Tracked(ctx, a, dag.file_slots, dag.leaf_ids)
    slots, old, new = dag.change_set(0.01)
    t.step(slots, new)
    es, ed = t.expect()
    assert len(es) >= 100
    rng = np.random.default_rng(17)
    KIND = 3
    assoc = capi.Assoc(ctx, 4096)
    hashes = np.repeat(HK.key_hash(ed), 3)
    fillers = HK.keys_with_hash(rng, hashes, len(hashes))
    assert (assoc.put(KIND, fillers, nonzero_vals(rng, len(fillers))) == 0).all()
    table = {ed[i].tobytes(): rng.integers(1, 256, size=32, dtype=np.uint8).tobytes() for i in range(0, len(es), 2)}
    assert (assoc.put(KIND, np.frombuffer(b"".join(table), np.uint8),
                      np.frombuffer(b"".join(table.values()), np.uint8)) == 0).all()
    assert 2 * assoc.stats()[0] <= assoc.stats()[1]
    cap = len(es)
    d_slots, d_keys, d_vals = ctx.alloc(4 * cap), ctx.alloc(32 * cap), ctx.alloc(32 * cap)
    d_status, d_n2 = ctx.alloc(cap), ctx.alloc(16)
    t.g.feed_lookup_device(None, assoc, KIND, cap, d_slots.ptr, d_keys.ptr, d_status.ptr, d_vals.ptr, d_n2.ptr)
    ctx.sync()
    assert d_n2.to_numpy(np.uint64).tolist() == [cap, cap]
    assert d_slots.to_numpy(np.uint32).tolist() == es.tolist()
    assert d_keys.to_numpy(np.uint8).tobytes() == ed.tobytes()
    vals, found = assoc.get(KIND, ed)
    assert d_status.to_numpy(np.uint8).tolist() == found.tolist() == [int(k.tobytes() in table) for k in ed]
    assert d_vals.to_numpy(np.uint8).tobytes() == vals.tobytes()
    assert rows_of(vals) == [table.get(k.tobytes(), ZERO) for k in ed]
    for b in (d_slots, d_keys, d_vals, d_status, d_n2):
        b.free()
    assoc.close()
    t.close()
