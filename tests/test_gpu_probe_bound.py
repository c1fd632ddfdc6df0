"""The documented probe bound (65536 slots), one test per table: 65536 keys of
one hash form a run the bound still admits -- the last key makes exactly 65536
probes -- and the 65537th does not fit.  Each case reaches an error return,
never a fault: every bounded loop exits by construction, and the unbounded
ones (assoc_find, k5_assoc_insert) are never entered with a batch the dedup
refused.  No table is ever more than half full.

  dedup (rf_dedup_digests)   RF_EDEVICE; the device form sets bit 31 of *d_n_unique
  assoc (rf_assoc_put)       RF_EDEVICE from its dedup step: the batch is not applied
  repository index           RF_EDEVICE from k9_put_insert, then fail-stop
  liveset (rf_liveset_run)   RF_EDEVICE: the run is not applied

Each case walks about 2^31 probe steps."""
import numpy as np
import pytest

import hashkeys as HK
import repo_model as RM
from reflow_amd import capi
from test_gpu_liveset_walk import Session, fileset, node

pytestmark = pytest.mark.gpu

H = HK.WRAP_HASH
BOUND = 1 << 16


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def refused(fn, *args):
    with pytest.raises(capi.RfError) as e:
        fn(*args)
    assert e.value.code == capi.RF_EDEVICE, e.value
    return e.value


def first_occurrence(d):
    first = {}
    return [first.setdefault(r.tobytes(), i) for i, r in enumerate(d)]


def test_dedup_bound(ctx):
    rng = np.random.default_rng(20)
    keys = HK.keys_with_hash(rng, H, BOUND + 1)
    canon, nu = ctx.dedup_digests(keys[:BOUND])
    assert nu == BOUND and canon.tobytes() == np.arange(BOUND, dtype=np.uint32).tobytes()
    refused(ctx.dedup_digests, keys)
    dd, dc, dn = ctx.upload(keys), ctx.alloc(4 * (BOUND + 1)), ctx.alloc(64)
    ctx.dedup_digests_device(dd.ptr, BOUND + 1, dc.ptr, dn.ptr)
    ctx.sync()
    assert int(dn.to_numpy(np.uint32, count=1)[0]) >> 31 == 1
    for b in (dd, dc, dn):
        b.free()
    # the context works afterwards
    d = rng.integers(0, 256, size=(300, 32), dtype=np.uint8)[rng.integers(0, 300, size=2000)]
    canon, nu = ctx.dedup_digests(d)
    want = first_occurrence(d)
    assert canon.tolist() == want and nu == len(set(want))


def test_assoc_put_bound(ctx):
    rng = np.random.default_rng(21)
    a = capi.Assoc(ctx, 1024)
    keys = np.concatenate([HK.keys_with_hash(rng, H, 60), rng.integers(0, 256, size=(60, 32), dtype=np.uint8)])
    vals = rng.integers(1, 256, size=(120, 32), dtype=np.uint8)
    assert (a.put(0, keys[:80], vals[:80]) == 0).all() and (a.put(5, keys[40:], vals[40:]) == 0).all()

    def state():
        k, v, kd = a.scan(-1)
        rows = sorted(zip(kd.tolist(), (r.tobytes() for r in k), (r.tobytes() for r in v)))
        return a.stats()[0], rows, [x.tobytes() for kind in (0, 5) for x in a.get(kind, keys)]

    before = state()
    assert before[0] == 160 and len(before[1]) == 160
    many = HK.keys_with_hash(rng, H, BOUND + 1)
    refused(a.put, 0, many, np.ones((BOUND + 1, 32), np.uint8))  # the batch is not applied
    assert state() == before  # (the capacity may have grown)
    more = HK.keys_with_hash(rng, H, 40)
    assert (a.put(0, more, vals[:40]) == 0).all()
    got, found = a.get(0, more)
    assert found.all() and got.tobytes() == vals[:40].tobytes() and a.stats()[0] == 200
    assert state()[2][:2] == before[2][:2]
    a.close()


def test_repo_index_bound_is_fail_stop(ctx):
    rng = np.random.default_rng(22)
    ids = HK.keys_with_hash(rng, H, 80000)
    r = capi.Repo(ctx)
    assert (r.put(ids[:40000], np.arange(40000)) == 0).all()  # (each batch's own dedup stays below the bound)
    assert r.stats().objects == 40000
    refused(r.put, ids[40000:], np.arange(40000))  # k9_put_insert: the run would pass 65536 slots
    refused(r.stat, ids[:10])
    refused(r.put, rng.integers(0, 256, size=(4, 32), dtype=np.uint8), np.ones(4, np.int64))
    refused(r.remove, ids[:10])
    refused(r.stats)
    r.close()
    fresh, model = capi.Repo(ctx), RM.Repo()  # a fresh index on the same context is unaffected
    some = [x.tobytes() for x in ids[:300]]
    assert fresh.put(RM.ids_array(some), list(range(300))).tolist() == model.put(some, list(range(300))).tolist()
    assert fresh.remove(RM.ids_array(some[::4])).tolist() == model.remove(some[::4]).tolist()
    assert fresh.stat(RM.ids_array(some)).tolist() == model.stat(some).tolist()
    st, want = fresh.stats(), model.stats()
    assert {k: getattr(st, k) for k in want} == want
    fresh.close()


def test_liveset_row_bound(ctx):
    rng = np.random.default_rng(23)
    sizes = np.arange(1, BOUND + 2, dtype=np.int64)
    ids = HK.rows_with_hash(rng, H, 0, sizes)  # one value, so ordinal 0: 65537 classes of one live_hash
    root = node(rows=list(zip((x.tobytes() for x in ids), sizes.tolist())))
    s = Session(ctx, [root])
    refused(s.L.run, [0])  # the run is not applied
    root.value = fileset([(rng.bytes(32), int(i % 7)) for i in range(40)] * 2)
    s.push([0])
    st, want = s.run([0])  # (compared with live_model in every figure, the filter's words included)
    assert (want.nlive_est, want.nlive) == (80, 40) and st.changed == 1
    s.close()
