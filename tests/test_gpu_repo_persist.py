"""The repository index read back out of HBM (rf_repo_scan / _collect_list /
_compact / _save / _restore, k9_repo.hip) against the object map of
tests/repo_model.py: the scan at the tile edges and under a cap, dense runs
built with tests/hashkeys.py across the table's end and a tile edge,
tombstones, collect_list against the oracle's bloom Contains in both forms and
all or nothing, compaction, and the file: round trips, equal contents giving
equal bytes (and the Python writer's bytes), damaged files, the fixture."""
import ctypes
import os

import numpy as np
import pytest

import hashkeys as HK
import live_model as LM
import reflow_oracle as O
import repo_model as M
import repo_persist_cases as C
from reflow_amd import capi

pytestmark = pytest.mark.gpu

POISON = C.POISON
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repo_v1.bin")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def keys(ids):
    return [bytes(r) for r in np.asarray(ids).reshape(-1, 32)]


def is_poison(*arrays):
    return all(a is None or a.tobytes() == bytes([POISON]) * a.nbytes for a in arrays)


class OracleBloom:
    """A filter built by rf_bloom_new + rf_bloom_add, and the oracle's bloomlive over the same adds."""

    def __init__(self, ctx, live, n_est):
        self.m, self.k = O.estimate_parameters(max(n_est, 1), 0.01)
        self.dev = capi.Bloom.new(ctx, self.m, self.k)
        self.words = np.zeros((self.m + 63) // 64, dtype=np.uint64)
        self.length = np.array([self.dev.params()[2]], dtype=np.uint64)
        if live:
            self.dev.add(M.ids_array(live))
            O.lib().orc_bloomlive_add_batch(self.words.ctypes.data, self.length.ctypes.data, self.m, self.k,
                                            b"".join(live), len(live))
        assert int(self.length[0]) == self.dev.params()[2]

    def contains_map(self, ids):
        out = np.zeros(max(len(ids), 1), dtype=np.uint8)
        if ids:
            O.lib().orc_bloomlive_contains_batch(self.words.ctypes.data, int(self.length[0]), self.m, self.k,
                                                 b"".join(ids), len(ids), out.ctypes.data, 1)
        return dict(zip(ids, out.astype(bool).tolist()))

    def close(self):
        self.dev.close()


def collect_list_device(ctx, repo, live, cap, ids=True, sizes=True):
    """(ids [cap, 32], sizes [cap], removed, removed_bytes) of the device form, outputs poisoned first."""
    d = C.DevList(ctx, cap, ids, sizes)
    repo.collect_list_device(live, cap, d.ids.ptr if ids else None, d.sizes.ptr if sizes else None, d.n.ptr,
                             d.nbytes.ptr)
    return d.read()


def run_collect_list(t, live, contains, device, all_ids):
    """One collect_list on the twin against the model; the removed ID -> size."""
    before_ids, _ = t.scan()
    dead = C.model_dead(t.ref, contains)
    st0 = t.dev.stats()
    cap = len(t.ref.objs)
    if device:
        ids, sizes, n, nb = collect_list_device(t.ctx, t.dev, live, cap)
    else:
        ids, sizes, n, nb, _ = t.dev.collect_list(live, cap=cap, poison=POISON)
    assert (n, nb) == (len(dead), sum(dead.values()))
    assert C.as_dict(ids[:n], sizes[:n]) == dead
    assert is_poison(ids[n:], sizes[n:])
    assert C.is_subsequence(keys(ids[:n]), keys(before_ids))  # ascending slot order
    assert t.ref.collect(contains) == (n, nb)
    st1 = t.dev.stats()
    assert (st0.objects - st1.objects, st0.bytes - st1.bytes, st1.tombstones - st0.tombstones) == (n, nb, n)
    t.scan()
    t.stat(all_ids)
    return dead


# ---- 7. scan edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049])
def test_scan_at_the_tile_edges(ctx, n):
    """A fresh index of 1024 slots: up to 512 objects stay in one tile, 513 give
    two, 1025 four and 2049 eight."""
    t = C.Twin(ctx, 0)
    ids, sizes = C.objects(np.random.default_rng(100 + n), n)
    t.put(ids, sizes)
    tiles = {0: 1, 1: 1, 255: 1, 256: 1, 257: 1, 511: 1, 512: 1, 513: 2, 1023: 2, 1024: 2, 1025: 4, 2049: 8}[n]
    assert t.dev.stats().capacity == tiles * capi.RF_REPO_LIST_TILE == t.ref.slots
    t.scan()
    t.close()


# ---- 8. cap slices -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world513(ctx):
    t = C.Twin(ctx, 0)
    t.put(*C.objects(np.random.default_rng(8), 513))
    full_ids, full_sizes = t.scan()
    yield t, full_ids, full_sizes
    t.close()


@pytest.mark.parametrize("cap", [0, 1, 512, 513, 514])
@pytest.mark.parametrize("want", ["both", "ids", "sizes"])
def test_scan_cap_slices(ctx, world513, cap, want):
    t, full_ids, full_sizes = world513
    wi, ws = want != "sizes", want != "ids"
    w = min(cap, 513)
    ids, sizes, n, rc = t.dev.scan(cap=cap, ids=wi, sizes=ws, poison=POISON, check=False)
    assert n == 513 and rc == (capi.RF_EINVAL if cap < 513 else capi.RF_OK)
    d_ids, d_sizes, d_n = C.scan_device(ctx, t.dev, cap, wi, ws)  # RF_OK: scan_device raises otherwise
    assert d_n == 513
    for got_ids, got_sizes in ((ids, sizes), (d_ids, d_sizes)):
        assert (got_ids is None) == (not wi) and (got_sizes is None) == (not ws)
        if wi:
            assert len(got_ids) == cap and got_ids[:w].tobytes() == full_ids[:w].tobytes() and is_poison(got_ids[w:])
        if ws:
            assert len(got_sizes) == cap and got_sizes[:w].tolist() == full_sizes[:w].tolist()
            assert is_poison(got_sizes[w:])


# ---- 9. dense runs across the table's end and a tile edge ----------------------------------------
def test_dense_run_wraps_the_table_and_crosses_a_tile_edge(ctx):
    """1100 IDs of one full hash in 4096 slots: the run starts at slot mask - 1,
    wraps the table's end and runs over the tile 0 / 1 boundary at slot 1024."""
    rng = np.random.default_rng(9)
    run = keys(HK.keys_with_hash(rng, HK.WRAP_HASH, 1100))
    assert (HK.key_hash(M.ids_array(run)) == HK.WRAP_HASH).all()
    sizes = [int(s) for s in rng.integers(0, 1 << 30, size=1100)]
    t = C.Twin(ctx, 2048)
    t.put(run, sizes)
    assert t.dev.stats().capacity == 4096
    t.scan()
    t.remove(run[::3])
    ids, _ = t.scan()
    assert t.dev.stats().tombstones == len(run[::3])
    rest = C.model_dead(t.ref, None)
    got_ids, got_sizes, n, nb, _ = t.dev.collect_list(None, poison=POISON)
    assert n == len(rest) == 1100 - len(run[::3]) and nb == sum(rest.values())
    assert C.as_dict(got_ids, got_sizes) == rest and keys(got_ids) == keys(ids)  # everything, in scan order
    t.ref.collect(None)
    t.scan()
    t.stat(run)
    t.close()


# ---- 10. tombstones ----------------------------------------------------------------------------
def test_scan_over_tombstones_and_revived_objects(ctx):
    rng = np.random.default_rng(10)
    ids, sizes = C.objects(rng, 1500)
    t = C.Twin(ctx, 0)
    t.put(ids, sizes)
    t.scan()
    gone = ids[::3]
    t.remove(gone)
    t.scan()
    assert t.dev.stats().tombstones == len(gone) == 500
    back = gone[::2]
    t.put(back, [s + 7 for s in sizes[::3][::2]])  # (live + tombstones + 250 rows stay within half the slots)
    t.scan()
    assert t.dev.stats().tombstones == len(gone) - len(back) == 250 and t.dev.stats().rebuilds == t.ref.rebuilds
    t.stat(ids)
    t.close()


# ---- 11. collect_list against the model ----------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_collect_list_against_the_oracles_bloom(ctx, device):
    rng = np.random.default_rng(11)
    ids, sizes = C.objects(rng, 2000)
    live = [ids[i] for i in np.random.default_rng(12).permutation(2000)[:1000].tolist()]
    b = OracleBloom(ctx, live, 2000)
    contains = b.contains_map(ids)
    assert all(contains[i] for i in live) and 900 <= sum(not c for c in contains.values()) <= 1000
    t = C.Twin(ctx, 0)
    t.put(ids, sizes)
    dead = run_collect_list(t, b.dev, lambda i: contains[i], device, ids)
    assert len(dead) == sum(not c for c in contains.values()) and not set(dead) & set(live)
    # nothing dead: removed == 0 and nothing written
    assert run_collect_list(t, b.dev, lambda i: contains[i], device, ids) == {}
    # everything dead: a nil liveset
    assert len(run_collect_list(t, None, None, device, ids)) == 2000 - len(dead)
    assert t.dev.stats().objects == 0
    # an empty index
    assert run_collect_list(t, None, None, device, ids) == {}
    assert run_collect_list(t, b.dev, lambda i: contains[i], device, ids) == {}
    e = C.Twin(ctx, 0)
    assert run_collect_list(e, None, None, device, ids[:10]) == {}
    e.close()
    t.close()
    b.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_collect_list_with_the_borrowed_filter(ctx, device):
    """TestGC (test/evaltest/eval_test.go:353-393): the liveset's own filter,
    lent by rf_liveset_filter; the removed set is rf_bloom_collect's dead set
    over the scanned IDs -- `unrooted`, and the extras the filter does not hold."""
    nodes, ix = LM.gc_flow()
    LM.gc_stage(nodes, ix, 3)
    fl = C.Flow(ctx, nodes)
    fl.L.run([ix["pullup"]])
    want_live = LM.live(nodes, [ix["pullup"]])
    gids, gsizes = LM.gc_objects()
    rng = np.random.default_rng(13)
    extra = [rng.bytes(32) for _ in range(600)]  # dead but for the filter's false positives
    all_ids = keys(gids) + extra
    all_sizes = gsizes.tolist() + [int(i[2]) for i in extra]
    t = C.Twin(ctx, 0)
    t.put(all_ids, all_sizes)
    b = fl.L.filter()
    scan_ids, scan_sizes = t.scan()
    dead_idx, dead_bytes = b.collect(scan_ids, scan_sizes)  # rf_bloom_collect over the scanned rows
    contains = dict(zip(all_ids, want_live.contains(all_ids)))
    dead = run_collect_list(t, b, lambda i: contains[i], device, all_ids)
    assert keys(scan_ids[dead_idx]) == [k for k in keys(scan_ids) if k in dead] and sum(dead.values()) == dead_bytes
    assert bytes(gids[7]) in dead and 590 < len(dead) <= 601
    fl.close()
    t.close()


# ---- 12. all or nothing ----------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_collect_list_is_all_or_nothing(ctx, device):
    rng = np.random.default_rng(12)
    ids, sizes = C.objects(rng, 40)
    live = ids[10:]
    b = OracleBloom(ctx, live, 1 << 14)  # (a large filter: no false positive among the ten)
    contains = b.contains_map(ids)
    assert [contains[i] for i in ids] == [False] * 10 + [True] * 30
    t, twin = C.Twin(ctx, 0), C.Twin(ctx, 0)
    for x in (t, twin):
        x.put(ids, sizes)
    before_ids, before_sizes = t.scan()
    st0 = t.dev.stats()
    for wi, ws in ((True, True), (True, False), (False, True)):
        if device:
            got_ids, got_sizes, n, nb = collect_list_device(ctx, t.dev, b.dev, 9, wi, ws)  # RF_OK: it raises otherwise
        else:
            got_ids, got_sizes, n, nb, rc = t.dev.collect_list(b.dev, cap=9, ids=wi, sizes=ws, poison=POISON,
                                                               check=False)
            assert rc == capi.RF_EINVAL
        assert n == 10 and nb == 0 and is_poison(got_ids, got_sizes)
        st1 = t.dev.stats()
        assert (st1.objects, st1.bytes, st1.tombstones) == (st0.objects, st0.bytes, st0.tombstones) == (40, sum(sizes), 0)
        ids2, sizes2 = t.scan()
        assert ids2.tobytes() == before_ids.tobytes() and sizes2.tobytes() == before_sizes.tobytes()
        t.stat(ids)
    # cap = 10 removes and lists all ten
    if device:
        got_ids, got_sizes, n, nb = collect_list_device(ctx, t.dev, b.dev, 10)
    else:
        got_ids, got_sizes, n, nb, _ = t.dev.collect_list(b.dev, cap=10, poison=POISON)
    assert n == 10 and nb == sum(sizes[:10]) and C.as_dict(got_ids, got_sizes) == dict(zip(ids[:10], sizes[:10]))
    assert keys(got_ids) == [k for k in keys(before_ids) if k in set(ids[:10])]
    assert t.ref.collect(lambda i: contains[i]) == (10, nb)
    t.scan()
    # both arrays NULL with cap = 0: a plain collect, as rf_repo_collect on the twin
    want = twin.dev.collect(b.dev)
    assert twin.ref.collect(lambda i: contains[i]) == want == (10, nb)
    p = C.Twin(ctx, 0)
    p.put(ids, sizes)
    if device:
        _, _, n, nb2 = collect_list_device(ctx, p.dev, b.dev, 0, False, False)
    else:
        _, _, n, nb2, _ = p.dev.collect_list(b.dev, cap=0, ids=False, sizes=False)
    assert (n, nb2) == want and p.ref.collect(lambda i: contains[i]) == want
    p.scan()
    twin.scan()
    for x in (t, twin, p, b):
        x.close()


# ---- 13. compact -------------------------------------------------------------------------------------
def test_compact(ctx):
    rng = np.random.default_rng(13)
    ids, sizes = C.objects(rng, 3000)
    t = C.Twin(ctx, 0)
    t.put(ids, sizes)
    gone = [ids[i] for i in rng.permutation(3000)[:1800].tolist()]
    t.remove(gone)
    before, rebuilds = C.as_dict(*t.scan()), t.dev.stats().rebuilds
    assert t.dev.stats().tombstones == 1800 and t.dev.stats().capacity == 8192
    t.compact()
    st = t.dev.stats()
    assert (st.tombstones, st.capacity, st.rebuilds, st.objects) == (0, M.slots_for(1200), rebuilds + 1, 1200)
    assert st.capacity == 4096
    assert C.as_dict(*t.scan()) == before
    t.stat(ids)
    t.compact(5000)  # min_capacity is honoured
    assert t.dev.stats().capacity == M.slots_for(5000) == 16384 and t.dev.stats().rebuilds == rebuilds + 2
    t.compact(0)
    assert t.dev.stats().capacity == 4096
    t.scan()
    # a Put batch large enough to grow, and removals, go on as the model does
    more_ids, more_sizes = C.objects(rng, 2500)
    t.put(more_ids + gone[:100], more_sizes + [1] * 100)
    assert t.dev.stats().capacity > 4096
    t.remove(more_ids[:50])
    t.scan()
    t.stat(ids + more_ids)
    t.close()
    # TestCacheLookupMissing's shape (test/evaltest/eval_test.go:279-312): x, y, z of one byte, x deleted
    c = C.Twin(ctx, 0)
    files = [(O.sha256(s), 1) for s in (b"x", b"y", b"z")]
    c.put([f[0] for f in files], [1, 1, 1])
    c.remove([files[0][0]])
    c.compact()
    counts, mids, msizes = M.flatten([files])
    want = c.ref.missing([files])
    got = c.dev.missing(counts, mids, msizes)
    assert got.n_missing.tolist() == want.n_missing.tolist() == [1] and got.n_files.tolist() == [3]
    assert got.missing_bytes.tolist() == [1] and keys(got.miss_ids32[:1]) == [files[0][0]] == want.ids
    C.check_stats(c.dev, c.ref)
    c.close()
    # an empty index
    e = C.Twin(ctx, 5000)
    e.compact()
    assert e.dev.stats().capacity == 1024 and e.dev.stats().rebuilds == 1
    e.scan()
    e.put(ids[:5], sizes[:5])
    e.scan()
    e.close()


# ---- 14. save / restore ----------------------------------------------------------------------------------
def test_save_restore_round_trip(ctx, tmp_path):
    rng = np.random.default_rng(14)
    ids, sizes = C.objects(rng, 1700)
    t = C.Twin(ctx, 0)
    t.put(ids, sizes)
    t.remove(ids[::4])
    path = tmp_path / "index.rfrepo"
    t.dev.save(path)
    assert not os.path.exists(str(path) + ".tmp")
    r = C.Twin.__new__(C.Twin)
    r.ctx, r.dev, r.ref = ctx, capi.Repo.restore(ctx, path), C.model_restored(t.ref.objs)
    st = r.dev.stats()
    assert (st.objects, st.bytes, st.tombstones, st.capacity, st.rebuilds) == (
        len(t.ref.objs), sum(t.ref.objs.values()), 0, M.slots_for(len(t.ref.objs)), 0)
    assert (st.last_rows, st.last_files, st.last_missing) == (0, 0, 0)
    r.scan()
    r.stat(ids)
    # the restored index goes on like any other
    new_ids, new_sizes = C.objects(rng, 900)
    r.put(new_ids + ids[:8], new_sizes + [3] * 8)
    r.remove(ids[1:200:2])
    r.scan()
    groups = [list(zip(ids[:30], sizes[:30])), list(zip(new_ids[:5], new_sizes[:5])) + [(rng.bytes(32), 9)]]
    counts, mids, msizes = M.flatten(groups)
    got, want = r.dev.missing(counts, mids, msizes), r.ref.missing(groups)
    assert got.n_missing.tolist() == want.n_missing.tolist() and got.n_listed == want.n_listed
    assert got.miss_ids32[:want.n_listed].tobytes() == want.miss_ids32.tobytes()
    b = OracleBloom(ctx, new_ids, 4000)
    contains = b.contains_map(list(r.ref.objs))
    run_collect_list(r, b.dev, lambda i: contains[i], False, ids + new_ids)
    b.close()
    r.close()
    t.scan()  # the saved index is as it was
    t.close()
    # an empty index saves and restores
    e = capi.Repo(ctx, 0)
    e.save(tmp_path / "empty.rfrepo")
    assert (tmp_path / "empty.rfrepo").read_bytes() == C.write_file([], [])
    e2 = capi.Repo.restore(ctx, tmp_path / "empty.rfrepo")
    assert e2.stats().objects == 0 and e2.stats().capacity == 1024 and e2.scan()[2] == 0
    assert e2.put(M.ids_array(ids[:3]), sizes[:3]).tolist() == [0, 0, 0] and e2.stats().objects == 3
    e.close()
    e2.close()


# ---- 15. equal contents, equal bytes ---------------------------------------------------------------------
def test_equal_contents_give_equal_files(ctx, tmp_path):
    rng = np.random.default_rng(15)
    ids, sizes = C.objects(rng, 1300)
    other_ids, other_sizes = C.objects(rng, 400)
    final = dict(zip(ids, sizes))
    # one batch
    a = capi.Repo(ctx, 0)
    a.put(M.ids_array(ids), sizes)
    # shuffled small batches with removals and re-Puts
    b = C.Twin(ctx, 0)
    order = rng.permutation(1300).tolist()
    for o in range(0, 1300, 97):
        part = order[o:o + 97]
        b.put([ids[i] for i in part] + other_ids[o % 400:o % 400 + 20],
              [sizes[i] for i in part] + other_sizes[o % 400:o % 400 + 20])
    b.remove(other_ids + ids[:300])
    b.put(ids[:300][::-1], sizes[:300][::-1])
    assert b.ref.objs == final and b.dev.stats().tombstones > 0
    # a larger initial capacity plus a compact
    c = C.Twin(ctx, 20000)
    c.put(other_ids + ids, other_sizes + sizes)
    c.remove(other_ids)
    c.compact()
    assert c.ref.objs == final and c.dev.stats().capacity == M.slots_for(1300) == 4096
    for name, r in (("a", a), ("b", b.dev), ("c", c.dev)):
        r.save(tmp_path / name)
    want = C.write_file(*C.sorted_arrays(final))  # the default chunk
    for name in "abc":
        assert (tmp_path / name).read_bytes() == want, name
    for r in (a, b, c):
        r.close()


# ---- 16. damaged files at restore ----------------------------------------------------------------------------
def test_restore_refuses_damaged_files_and_the_context_goes_on(ctx, tmp_path):
    ids, sizes = C.sorted_arrays(dict(zip(*C.objects(np.random.default_rng(16), 7))))
    ids, sizes = keys(ids), sizes.tolist()
    good = C.write_file(ids, sizes, 80)

    def flip(byte):
        g = bytearray(good)
        g[byte] ^= 0x10
        return bytes(g)

    cases = {
        "truncated": (good[:-1], capi.RF_EINVAL),
        "cut in the entries": (good[:200], capi.RF_EINVAL),
        "empty": (b"", capi.RF_EINVAL),
        "trailing byte": (good + b"\0", capi.RF_EINVAL),
        "entry bit": (flip(64 + 45), capi.RF_EINTEGRITY),
        "digest bit": (flip(64 + 280 + 3), capi.RF_EINTEGRITY),
        "total_bytes bit": (flip(33), capi.RF_EINTEGRITY),
        "magic bit": (flip(2), capi.RF_EINVAL),
        "reserved bit": (flip(50), capi.RF_EINVAL),
        "end marker bit": (flip(len(good) - 2), capi.RF_EINVAL),
        "equal IDs": (C.write_file(ids[:3] + [ids[2]] + ids[4:], sizes, 80), capi.RF_EINVAL),
        "descending IDs": (C.write_file(ids[::-1], sizes, 80), capi.RF_EINVAL),
        "negative size": (C.write_file(ids, sizes[:6] + [-4], 80), capi.RF_EINVAL),
        "total off by one": (C.write_file(ids, sizes, 80, total=sum(sizes) + 1), capi.RF_EINVAL),
        "sizes overflow": (C.write_file(ids, [2 ** 63 - 1] * 2 + sizes[2:], 80), capi.RF_EINVAL),
    }
    for what, (data, want) in cases.items():
        path = tmp_path / "bad.rfrepo"
        path.write_bytes(data)
        out = ctypes.c_void_p(0x1234)  # *out is untouched
        rc = capi.lib().rf_repo_restore(ctx.handle, os.fsencode(path), ctypes.byref(out))
        assert (rc, out.value) == (want, 0x1234), what
    out = ctypes.c_void_p(0x1234)
    rc = capi.lib().rf_repo_restore(ctx.handle, os.fsencode(tmp_path / "absent"), ctypes.byref(out))
    assert (rc, out.value) == (capi.RF_EIO, 0x1234)
    # the same context restores the good file and answers a Stat
    (tmp_path / "good.rfrepo").write_bytes(good)
    r = capi.Repo.restore(ctx, tmp_path / "good.rfrepo")
    assert r.stat(M.ids_array(ids + [bytes(32)])).tolist() == sizes + [-1]
    r.close()


# ---- 17. the fixture on the device ------------------------------------------------------------------------
def test_the_golden_fixture_restores(ctx):
    r = capi.Repo.restore(ctx, FIXTURE)
    ids, sizes, n, _ = r.scan()
    assert n == 5 and C.as_dict(ids, sizes) == dict(zip(C.GOLDEN_IDS, C.GOLDEN_SIZES))
    st = r.stats()
    assert (st.objects, st.bytes, st.tombstones, st.capacity) == (5, sum(C.GOLDEN_SIZES), 0, 1024)
    assert r.stat(M.ids_array(C.GOLDEN_IDS)).tolist() == C.GOLDEN_SIZES
    r.close()
