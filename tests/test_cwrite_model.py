"""The cache write's CPU model (tests/cwrite_model.py) on its own: the
participation rule on hand-built rows, the tables' ordering rules, and what
the seeded scenarios that tests/test_gpu_cache_write.py replays on the device
cover -- every skip reason, a participating node whose physical key is absent,
two nodes of one batch sharing a key, a node listed twice."""
import pytest

import cwrite_model as M
import reflow_oracle as O
import wave_model as W

K1, K2 = O.sha256(b"key 1"), O.sha256(b"key 2")
F1, F2 = O.sha256(b"fsid 1"), O.sha256(b"fsid 2")


def test_participation_rule():
    c, x, inv = W.F_CACHEABLE, W.F_EXTERN, W.F_INVALID
    assert M.participation(0, [K1], False) == (M.NOT_CACHEABLE, [])
    assert M.participation(x, [K1], True) == (M.NOT_CACHEABLE, [])          # the first reason that holds
    assert M.participation(c | x, [K1], True) == (M.EXTERN, [])
    assert M.participation(c | x, [K1], False) == (M.WRITTEN, [K1])
    assert M.participation(c, [], False) == (M.NO_KEY, [])
    assert M.participation(c, [W.ZERO], False) == (M.NO_KEY, [])
    assert M.participation(c, [W.ZERO, K2], False) == (M.WRITTEN, [K2])     # an absent physical key
    assert M.participation(c | inv, [K1, K2], False) == (M.WRITTEN, [K1, K2])  # INVALID does not matter for a write


def test_tables_order_and_refusal():
    t = M.Tables()
    flags = [W.F_CACHEABLE] * 3
    keys = [[K1, K2], [K2], [K1]]
    done = [W.DONE] * 3
    out = t.write(flags, done, keys, [0, 1], [F1, F2], [10, 20])
    assert out == (2, 3, [0, 0, 0], [2, 1])
    assert t.assoc_entries() == {K1: F1, K2: F2} and t.repo == {F1: 10, F2: 20}   # the later writer of K2 stays
    # a node listed twice takes part twice, in order; the first size of an fsid stays
    out = t.write(flags, done, keys, [2, 2], [F2, F1], [99, 10])
    assert out == (2, 2, [0, 0, 0], [1, 1]) and t.assoc[M.KIND, K1] == F1 and t.repo[F2] == 20
    before = (dict(t.assoc), dict(t.repo))
    with pytest.raises(M.Refused):
        t.write(flags, [W.DONE, W.READY, W.DONE], keys, [0, 1], [F1, F2], [10, 20])
    assert (t.assoc, t.repo) == before
    # without a repository only the assoc moves
    t.write(flags, done, keys, [1], [O.sha256(b"fsid 3")], [5], repo=False)
    assert len(t.repo) == 2 and t.assoc[M.KIND, K2] == O.sha256(b"fsid 3")


@pytest.fixture(scope="module")
def played():
    out = []
    for seed, n, nce in M.SEEDS:
        case = M.CwCase(seed, n)
        target = M.ModelTarget(case)
        out.append((nce, case, target, M.play(case, target, no_cache_extern=nce)))
    return out


def test_seeds_cover_the_write(played):
    reasons = set()
    for nce, case, target, seen in played:
        reasons |= seen["reasons"]
        assert seen["batches"] >= 3 and seen["twice"] >= 1, (nce, seen)
        assert (M.EXTERN in seen["reasons"]) == nce, seen
        assert all(target.model.states[r] == W.DONE for r in case.roots)
        # the written entries are what the model's tables hold: every key maps to the fsid of a node that ran
        fsids = {O.sha256(M.value_of(i).json()) for i in seen["ran"]}
        assert set(target.tables.assoc_entries().values()) <= fsids
        assert set(target.tables.repo) <= fsids and len(target.tables.repo) > 0
    assert reasons == {M.WRITTEN, M.NOT_CACHEABLE, M.EXTERN, M.NO_KEY}
    assert sum(seen["absent_physical"] for _, _, _, seen in played) >= 2
    assert sum(seen["shared_key"] for _, _, _, seen in played) >= 1
    assert sum(seen["late_hits"] for _, _, _, seen in played) >= 1   # a write of this run served a later wave
    assert {nce for nce, _, _, _ in played} == {False, True}


def test_counters_add_up(played):
    for _, _, target, _ in played:
        for written, puts, skipped, per in target.outs:
            assert written + sum(skipped) == len(per) and puts == sum(per)
            assert written == sum(1 for k in per if k)
