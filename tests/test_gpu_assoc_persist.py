"""The HBM assoc's enumeration, compaction and save / restore
(rf_assoc_count / _scan / _scan_device / _compact / _save / _restore): what
the table holds is checked against the oracle's restatement of the in-memory
assoc (reflow_oracle.InmemoryAssoc, test/testutil/assoc.go:34-56), whose .m
dict is the expected content."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import reflow_oracle as O

pytestmark = pytest.mark.gpu
ZERO = bytes(32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # guard rows after the device form's output buffers


@pytest.fixture(scope="module")
def ctx():
    from reflow_amd import capi
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def rows(kinds, keys, vals):
    """Entries as a sorted array of 68-byte records (kind, key, value)."""
    n = len(kinds)
    rec = np.zeros((n, 68), dtype=np.uint8)
    rec[:, :4] = np.ascontiguousarray(kinds, dtype="<i4").view(np.uint8).reshape(n, 4)
    rec[:, 4:36] = np.asarray(keys, dtype=np.uint8).reshape(n, 32)
    rec[:, 36:] = np.asarray(vals, dtype=np.uint8).reshape(n, 32)
    return np.sort(rec.view("V68").reshape(n))


def ref_rows(ref, kind=-1):
    items = [(kd, k, v) for (kd, k), v in ref.m.items() if kind < 0 or kd == kind]
    return rows([i[0] for i in items], np.frombuffer(b"".join(i[1] for i in items), np.uint8),
                np.frombuffer(b"".join(i[2] for i in items), np.uint8))


def scan_rows(a, kind=-1):
    keys, vals, kinds = a.scan(kind)
    return rows(kinds, keys, vals)


def same(x, y):
    return len(x) == len(y) and bool((x == y).all())


def no_duplicates(r):
    return len(r) < 2 or bool((r[1:].view(np.uint8).reshape(-1, 68)[:, :36] !=
                               r[:-1].view(np.uint8).reshape(-1, 68)[:, :36]).any(axis=1).all())


def put_both(a, ref, kind, keys, vals, expect=None):
    """One Put batch into the assoc and the oracle; statuses must agree."""
    from reflow_amd import capi
    st = a.put(kind, keys, vals, expect)
    k, v = np.asarray(keys).reshape(-1, 32), np.asarray(vals).reshape(-1, 32)
    e = None if expect is None else np.asarray(expect).reshape(-1, 32)
    want = [ref.put(kind, None if e is None else e[i].tobytes(), k[i].tobytes(), v[i].tobytes())
            for i in range(len(k))]
    names = {capi.RF_OK: "ok", capi.RF_EPRECONDITION: "precondition"}
    assert [names[int(x)] for x in st] == want
    return st


def check_gets(a, ref, kind, keys):
    got, found = a.get(kind, keys)
    k = np.asarray(keys).reshape(-1, 32)
    want = [ref.get(kind, k[i].tobytes()) for i in range(len(k))]
    assert found.astype(bool).tolist() == [w is not None for w in want]
    assert got.tobytes() == b"".join(w or ZERO for w in want)


def check_scan_and_count(a, ref):
    for kind in (0, 1, -1):
        keys, vals, kinds = a.scan(kind)
        r = rows(kinds, keys, vals)
        want = ref_rows(ref, kind)
        assert no_duplicates(r), "kind %d: a key twice" % kind
        assert same(r, want), "kind %d: scan differs from the oracle" % kind
        if kind >= 0:
            assert (kinds == kind).all()
        live, deleted = a.count(kind)
        assert live == len(want) == len(keys)
        if kind < 0:
            assert live + deleted == a.stats()[0]
        again = a.scan(kind)  # an unchanged table scans the same, row for row
        assert all((x == y).all() for x, y in zip((keys, vals, kinds), again))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_scan_equals_oracle_after_every_batch(ctx, seed):
    """The mixed workload of test_assoc_batches_match_inmemory: a 300-key pool,
    two kinds, CAS, deletes, re-inserts, several growths."""
    from reflow_amd import capi
    rng = random.Random(seed)
    pool = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(300)]
    vals = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(50)]
    a = capi.Assoc(ctx, capacity=16)
    ref = O.InmemoryAssoc()
    check_scan_and_count(a, ref)
    for b in range(12):
        kind = b % 2
        n = rng.choice([1, 7, 500, 3000])
        keys, vs, exps = [], [], []
        for _ in range(n):
            k = rng.choice(pool)
            v = ZERO if rng.random() < 0.1 else rng.choice(vals)
            r = rng.random()
            cur = ref.get(kind, k)
            e = ZERO if r < 0.5 else (cur or ZERO) if r < 0.7 else rng.choice(vals)
            keys.append(k)
            vs.append(v)
            exps.append(e)
        put_both(a, ref, kind, np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(vs), np.uint8),
                 np.frombuffer(b"".join(exps), np.uint8) if b % 3 != 0 else None)
        check_scan_and_count(a, ref)
    a.close()


def scan_device(ctx, a, kind, cap_entries, with_kinds=True, stream_ctx=None):
    """rf_assoc_scan_device into buffers with GUARD guard rows of 0xA5 after
    cap_entries; returns (n, keys, vals, kinds) of the rows written and
    asserts the guards."""
    from reflow_amd import capi
    nrows = cap_entries + GUARD
    dk, dv = capi.DeviceBuffer(ctx, 32 * nrows), capi.DeviceBuffer(ctx, 32 * nrows)
    dkd, dn = capi.DeviceBuffer(ctx, 4 * nrows), capi.DeviceBuffer(ctx, 8)
    for d in (dk, dv, dkd, dn):
        d.fill(0xA5)
    ctx.sync()
    a.scan_device(kind, cap_entries, dk.ptr, dv.ptr, dkd.ptr if with_kinds else None, dn.ptr,
                  stream_ctx.stream if stream_ctx else None)
    (stream_ctx or ctx).sync()
    n = int(dn.to_numpy(np.uint64)[0])
    keys, vals, kinds = dk.to_numpy().reshape(nrows, 32), dv.to_numpy().reshape(nrows, 32), dkd.to_numpy(np.int32)
    w = min(n, cap_entries)
    assert (keys[w:] == 0xA5).all() and (vals[w:] == 0xA5).all(), "rows past cap_entries / n written"
    assert (kinds[w if with_kinds else 0:].view(np.uint8) == 0xA5).all()
    for d in (dk, dv, dkd, dn):
        d.free()
    return n, keys[:w], vals[:w], kinds[:w]


@pytest.mark.parametrize("n", [0, 1, 512, 65000])
def test_scan_edges(ctx, n):
    """512 keys into capacity=512: a 1,024-slot table at exactly half load,
    smaller than one tile of the scan; 65,000 keys span many tiles."""
    from reflow_amd import capi
    rng = np.random.default_rng(n + 11)
    keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    vals = rng.integers(1, 256, size=(n, 32), dtype=np.uint8)
    a = capi.Assoc(ctx, capacity=512)
    if n:
        assert (a.put(0, keys[:n // 2], vals[:n // 2]) == 0).all()
        assert (a.put(3, keys[n // 2:], vals[n // 2:]) == 0).all()
    if n == 512:
        assert a.stats() == (512, 1024)
    kinds = np.where(np.arange(n) < n // 2, 0, 3).astype(np.int32)
    want = rows(kinds, keys, vals)
    assert a.count(-1) == (n, 0) and a.count(0) == (n // 2, 0) and a.count(3) == (n - n // 2, 0)
    k, v, kd = a.scan(-1, cap_entries=n)  # cap_entries == live
    assert same(rows(kd, k, v), want)
    for cap in sorted({max(n - 1, 0), 0} if n else set()):
        with pytest.raises(capi.RfError) as ei:
            a.scan(-1, cap_entries=cap)
        assert ei.value.code == capi.RF_EINVAL and ei.value.needed == n
    # kinds == NULL: fine for one kind, refused for every kind
    cnt = ctypes.c_uint64(0)
    kb, vb = np.zeros((max(n, 1), 32), np.uint8), np.zeros((max(n, 1), 32), np.uint8)
    rc = capi.lib().rf_assoc_scan(a._h, 3, n, kb.ctypes.data, vb.ctypes.data, None, ctypes.byref(cnt))
    assert rc == capi.RF_OK and cnt.value == n - n // 2
    assert same(rows(np.full(cnt.value, 3), kb[:cnt.value], vb[:cnt.value]), rows(kinds[n // 2:], keys[n // 2:], vals[n // 2:]))
    assert capi.lib().rf_assoc_scan(a._h, -1, n, kb.ctypes.data, vb.ctypes.data, None,
                                    ctypes.byref(cnt)) == capi.RF_EINVAL
    d8 = capi.DeviceBuffer(ctx, 64)
    assert capi.lib().rf_assoc_scan_device(a._h, -1, 1, d8.ptr, d8.ptr, None, d8.ptr, None) == capi.RF_EINVAL
    d8.free()
    # device form: exactly the host form's rows, nothing past cap_entries
    other = capi.Context(0, host_threads=0) if n == 65000 else None  # a caller's stream
    got_n, dk, dv, dkd = scan_device(ctx, a, -1, n, stream_ctx=other)
    assert got_n == n and (dk == k).all() and (dv == v).all() and (dkd == kd).all()
    for cap in sorted({max(n - 1, 0), 0}):
        got_n, dk, dv, dkd = scan_device(ctx, a, -1, cap)
        assert got_n == n and (dk == k[:cap]).all() and (dv == v[:cap]).all() and (dkd == kd[:cap]).all()
    got_n, dk, dv, _ = scan_device(ctx, a, 0, n // 2, with_kinds=False)
    assert got_n == n // 2 and same(rows(np.zeros(n // 2), dk, dv), rows(kinds[:n // 2], keys[:n // 2], vals[:n // 2]))
    if n == 65000:  # a growth right after a scan on the caller's stream frees the table it read only after it
        nrows = n + GUARD
        bufs = [capi.DeviceBuffer(ctx, 32 * nrows), capi.DeviceBuffer(ctx, 32 * nrows),
                capi.DeviceBuffer(ctx, 4 * nrows), capi.DeviceBuffer(ctx, 8)]
        ctx.sync()
        a.scan_device(-1, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, other.stream)
        more = rng.integers(0, 256, size=(70000, 32), dtype=np.uint8)
        assert (a.put(0, more, more | 1) == 0).all()
        other.sync()
        assert a.stats()[1] > 131072
        assert (bufs[0].to_numpy()[:32 * n].reshape(n, 32) == k).all()
        assert (bufs[1].to_numpy()[:32 * n].reshape(n, 32) == v).all()
        for d in bufs:
            d.free()
    a.close()
    if other:
        other.close()


def test_compaction(ctx):
    from reflow_amd import capi
    rng = np.random.default_rng(77)
    n = 50_000
    keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    vals = rng.integers(1, 256, size=(n, 32), dtype=np.uint8)
    a = capi.Assoc(ctx, capacity=16)
    ref = O.InmemoryAssoc()
    empty = capi.Assoc(ctx)
    empty.compact()
    assert empty.stats() == (0, 1024) and empty.count() == (0, 0)
    empty.close()
    half = n // 2
    put_both(a, ref, 0, keys[:half], vals[:half])
    put_both(a, ref, 1, keys[half:], vals[half:])
    dead = np.concatenate([np.arange(0, 22_500), np.arange(half, half + 22_500)])
    put_both(a, ref, 0, keys[:22_500], np.zeros((22_500, 32), np.uint8))
    put_both(a, ref, 1, keys[half:half + 22_500], np.zeros((22_500, 32), np.uint8))
    assert len(dead) == 45_000 and a.stats()[0] == n and a.count() == (5_000, 45_000)
    # a Get queued on another stream just before the compaction reads the old table
    other = capi.Context(0, host_threads=0)
    dk, dv, df = capi.DeviceBuffer(ctx, 32 * half), capi.DeviceBuffer(ctx, 32 * half), capi.DeviceBuffer(ctx, half)
    dk.copy_from(keys[:half])
    dv.fill(0xA5)
    df.fill(0xA5)
    ctx.sync()
    a.get_device(0, dk.ptr, half, dv.ptr, df.ptr, other.stream)
    a.compact(0)
    other.sync()
    want_v, want_f = vals[:half].copy(), np.ones(half, np.uint8)
    want_v[:22_500], want_f[:22_500] = 0, 0
    assert (df.to_numpy() == want_f).all() and (dv.to_numpy().reshape(half, 32) == want_v).all()
    for d in (dk, dv, df):
        d.free()
    other.close()
    assert a.stats() == (5_000, 16_384) and a.count() == (5_000, 0)
    for kind in (0, 1):
        check_gets(a, ref, kind, keys)
    # compare-and-set on a key that compaction dropped: its value is still "none"
    st = put_both(a, ref, 0, keys[:3], vals[:3], expect=vals[:3])
    assert (st == capi.RF_EPRECONDITION).all()
    fresh = rng.integers(0, 256, size=(100_000, 32), dtype=np.uint8)
    fvals = rng.integers(1, 256, size=(100_000, 32), dtype=np.uint8)
    put_both(a, ref, 1, fresh, fvals)  # growth after a compaction
    live, deleted = a.count()  # (the refused compare-and-sets may have claimed slots for their keys)
    assert live == 105_000 and live + deleted == a.stats()[0]
    for kind in (0, 1):
        check_gets(a, ref, kind, keys)
    check_gets(a, ref, 1, fresh)
    before = scan_rows(a)
    assert same(before, ref_rows(ref))
    a.compact(100_000)
    assert a.stats()[1] >= 200_000 and a.stats() == (105_000, 262_144)
    assert same(scan_rows(a), before)
    check_gets(a, ref, 1, fresh)
    a.close()


def mixed_batch(rng, a, ref, keys):
    """Overwrites, deletes, CAS hits and misses over known keys, two kinds."""
    n = len(keys)
    for kind in (0, 1):
        vals = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        vals[rng.random(n) < 0.2] = 0
        exp = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        exp[rng.random(n) < 0.5] = 0
        put_both(a, ref, kind, keys, vals, exp)
        check_gets(a, ref, kind, keys)


def test_save_restore_round_trip(ctx, tmp_path):
    from reflow_amd import capi
    rng = np.random.default_rng(5)
    n = 20_000
    keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    vals = rng.integers(1, 256, size=(n, 32), dtype=np.uint8)
    a = capi.Assoc(ctx, capacity=16)
    ref = O.InmemoryAssoc()
    put_both(a, ref, 0, keys[:12_000], vals[:12_000])
    put_both(a, ref, 1, keys[8_000:], vals[8_000:])
    put_both(a, ref, 0, keys[:3_000], np.zeros((3_000, 32), np.uint8))
    path = str(tmp_path / "assoc.bin")
    a.save(path)
    assert not os.path.exists(path + ".tmp")
    data = open(path, "rb").read()
    live = len(ref.m)
    assert live == 21_000 and len(data) == 64 + 68 * live + 32 + 40
    fk, fkeys, fvals = capi.assoc_file_parse(data)
    assert (rows(fk, fkeys, fvals).view(np.uint8).reshape(-1, 68) ==
            np.frombuffer(data[64:64 + 68 * live], np.uint8).reshape(-1, 68)).all(), "file entries not ascending"
    b = capi.Assoc.restore(ctx, path)
    assert same(scan_rows(b), scan_rows(a)) and same(scan_rows(b), ref_rows(ref))
    assert b.stats() == (live, 65_536) and b.count() == (live, 0)
    mixed_batch(rng, b, ref, keys[::7])
    assert same(scan_rows(b), ref_rows(ref))
    a.close()
    b.close()


def test_equal_contents_save_identical_files(ctx, tmp_path):
    """One table built in shuffled order from capacity=16 with 1,000 extra keys
    put and deleted, the other in one batch per kind from capacity=1<<17 -- and
    on a context with host threads, whose save sorts and hashes on the pool
    (the module's context has none)."""
    from reflow_amd import capi
    rng = np.random.default_rng(6)
    n = 40_000
    keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    vals = rng.integers(1, 256, size=(n, 32), dtype=np.uint8)
    extra = rng.integers(0, 256, size=(1_000, 32), dtype=np.uint8)
    a = capi.Assoc(ctx, capacity=16)
    order = rng.permutation(n)
    assert (a.put(1, extra, extra | 1) == 0).all()
    for part in np.array_split(order, 9):
        for kind in (0, 1):
            sel = part[part % 2 == kind]
            assert (a.put(kind, keys[sel], vals[sel] ^ 0xff) == 0).all()  # a first value, overwritten below
            assert (a.put(kind, keys[sel], vals[sel]) == 0).all()
    assert (a.put(1, extra, np.zeros_like(extra)) == 0).all()
    threaded = capi.Context(0)
    b = capi.Assoc(threaded, capacity=1 << 17)
    for kind in (0, 1):
        assert (b.put(kind, keys[kind::2], vals[kind::2]) == 0).all()
    assert a.stats() != b.stats()
    pa, pb = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    a.save(pa)
    b.save(pb)
    da = open(pa, "rb").read()
    assert da == open(pb, "rb").read()
    assert len(da) == 64 + 68 * n + 32 + 40
    c = capi.Assoc.restore(threaded, pa)  # (checksums on the pool)
    assert same(scan_rows(c), scan_rows(a))
    for x in (a, b, c):
        x.close()
    threaded.close()


def test_damaged_files_are_refused_and_the_context_survives(ctx, tmp_path):
    from reflow_amd import capi
    rng = np.random.default_rng(8)
    keys = rng.integers(0, 256, size=(2_000, 32), dtype=np.uint8)
    vals = rng.integers(1, 256, size=(2_000, 32), dtype=np.uint8)
    a = capi.Assoc(ctx)
    assert (a.put(0, keys, vals) == 0).all()
    path = str(tmp_path / "assoc.bin")
    a.save(path)
    data = open(path, "rb").read()
    flipped = bytearray(data)
    flipped[64 + 68 * 1_234 + 50] ^= 0x04
    cases = [(bytes(flipped), capi.RF_EINTEGRITY), (data[:-1], capi.RF_EINVAL), (data[:64 + 68 * 700], capi.RF_EINVAL),
             (data[:10], capi.RF_EINVAL), (b"", capi.RF_EINVAL)]
    for i, (bad, code) in enumerate(cases):
        p = str(tmp_path / ("bad%d.bin" % i))
        open(p, "wb").write(bad)
        h = ctypes.c_void_p(0xDEAD0)
        assert capi.lib().rf_assoc_restore(ctx.handle, os.fsencode(p), ctypes.byref(h)) == code, i
        assert h.value == 0xDEAD0, "*out written on failure"
        assert len(capi.lib().rf_last_error()) > 0
    h = ctypes.c_void_p(0xDEAD0)
    assert capi.lib().rf_assoc_restore(ctx.handle, os.fsencode(str(tmp_path / "missing.bin")),
                                       ctypes.byref(h)) == capi.RF_EIO and h.value == 0xDEAD0
    # the context and the assoc go on working
    assert (a.put(0, keys[:10], vals[10:20]) == 0).all()
    got, found = a.get(0, keys[:10])
    assert found.all() and (got == vals[10:20]).all()
    b = capi.Assoc.restore(ctx, path)
    got, found = b.get(0, keys)
    assert found.all() and (got == vals).all()
    a.close()
    b.close()


def test_golden_fixture_restores(ctx):
    from reflow_amd import capi
    from test_assoc_file import FIXTURE, fixture_entries
    a = capi.Assoc.restore(ctx, FIXTURE)
    assert a.stats() == (5, 1024)
    for kind, key, val in fixture_entries():
        got, found = a.get(kind, np.frombuffer(key, np.uint8))
        assert found[0] and got[0].tobytes() == val
        _, other = a.get(1 - kind, np.frombuffer(key, np.uint8))
        assert not other[0]
    a.close()


def test_host_mirror_assoc_persistence():
    """tests/cpp/assoc_persist_test: Assoc::Count / Scan / Compact / Save /
    Restore of include/reflow_host.hpp against a std::map model."""
    exe = os.path.join(ROOT, "tests", "cpp", "assoc_persist_test")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "PASS"
