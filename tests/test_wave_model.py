"""The evaluation waves' CPU model (tests/wave_model.py) against the
reference's bottom-up behavioural tests (test/evaltest/eval_test.go),
reduced to static graphs: which flows run and which are cache hits, every
root done at the end, every node in exactly one wave.  Also the two facts
that set bottom-up lookups apart from the top-down plan, the hand-over from
a plan's states, and what the seeded scenarios of tests/wave_cases.py cover
(tests/test_gpu_wave.py replays them on the device)."""
import numpy as np
import pytest

import plan_model as P
import reflow_oracle as O
import wave_cases as C
import wave_model as W

KIND = 0


def _cache(assoc, nodes, which, logical_only=True):
    """testutil.WriteCache: a value under the node's (logical) digest."""
    for i in which:
        for k in (W.wave_keys([nodes[i]])[0][-1:] if logical_only else
                  [k for k in W.wave_keys([nodes[i]])[0] if k != W.ZERO]):
            assoc.put(KIND, None, k, P.fileset_id(i))


def _evaluate(nodes, roots, assoc, accept=lambda i: True, nce=False, write_cache=False):
    """A complete bottom-up evaluation.  Returns (the model, the nodes that ran,
    node -> the (state, which) it was resolved to)."""
    w = W.Wave(nodes)
    resolved = {}

    def note():
        for i in w.last:
            assert i not in resolved  # never looked up twice (eval.go:906-917)
            resolved[i] = (int(w.states[i]), w.hits[i][0] if w.states[i] == W.HIT else None)

    def finish(done):
        for i in done:
            nodes[i].done = True
            if nodes[i].value is None:
                nodes[i].value = W.files("out%d" % i)
            if write_cache:
                _cache(assoc, nodes, [i], logical_only=False)
        return assoc, KIND, W.wave_keys(nodes), None

    w.begin(roots, assoc, KIND, W.wave_keys(nodes), no_cache_extern=nce)
    note()
    ran = []
    while w.last:
        hits = [int(i) for i in w.list(W.HIT, W.LAST)[0]]
        bad = [i for i in hits if not accept(i)]
        if bad:
            w.reject(bad)
        ready = [int(i) for i in w.list(W.READY, W.LAST)[0]]
        ran.extend(ready)
        w.step(sorted(set(hits) | set(ready)), *finish(sorted(set(hits) | set(ready))))
        note()
    # every root is done, nothing is left over, each node entered exactly one wave
    assert all(w.states[r] == W.DONE for r in roots)
    assert w.counts()[W.TODO] == w.counts()[W.READY] == w.counts()[W.HIT] == 0
    flat = [i for wave in w.history for i in wave]
    assert len(flat) == len(set(flat)) and set(flat) == set(resolved)
    return w, ran, resolved


def _executed(nodes, ran):
    """What went to the executor: the OpIntern / OpExec / OpExtern nodes that ran."""
    return {i for i in ran if P.flow_flags([nodes[i]])[0] & P.F_CACHEABLE}


def test_cache_lookup_bottomup():
    """TestCacheLookupBottomup (:232-277): "a" gets a cache hit, "b" a miss;
    the extern and exec(b) run."""
    nodes, ix = W.cache_lookup_bottomup_flow()
    assoc = O.InmemoryAssoc()
    _cache(assoc, nodes, [ix["intern"], ix["exec_a"]])
    w, ran, resolved = _evaluate(nodes, [ix["extern"]], assoc)
    assert _executed(nodes, ran) == {ix["extern"], ix["exec_b"]}
    assert resolved[ix["intern"]] == (W.HIT, 0)
    assert resolved[ix["exec_a"]] == (W.HIT, 1)  # its physical key is computable and misses; the logical one hits
    assert resolved[ix["exec_b"]] == (W.READY, None)
    assert w.history[0] == sorted([ix["intern"], ix["exec_a"], ix["exec_b"]])  # wave 0: no pending deps
    assert w.states[ix["val_a"]] == W.DONE and ix["val_a"] not in resolved     # flagged done: never in a wave
    # the waves follow the longest path to each node
    assert [len(x) for x in w.history] == [3, 1, 1, 1, 1, 0]


def test_cache_lookup_missing():
    """TestCacheLookupMissing (:279-312): the exec's cache entry exists but an
    object of its fileset does not -- the caller rejects the hit and the exec runs."""
    nodes, ix = W.cache_lookup_missing_flow()
    assoc = O.InmemoryAssoc()
    _cache(assoc, nodes, [ix["intern"], ix["exec"]])
    w, ran, resolved = _evaluate(nodes, [ix["exec"]], assoc, accept=lambda i: i != ix["exec"])
    assert resolved[ix["exec"]][0] == W.HIT and _executed(nodes, ran) == {ix["exec"]}
    # with every object present nothing runs
    nodes, ix = W.cache_lookup_missing_flow()
    w, ran, _ = _evaluate(nodes, [ix["exec"]], assoc)
    assert _executed(nodes, ran) == set()


def test_no_cache_extern_bottomup():
    """TestNoCacheExtern (:314-351), bottom-up: both execs and the extern run,
    the extern even though its keys are cached (eval.go:1173)."""
    nodes, ix = W.cache_lookup_bottomup_flow()
    assoc = O.InmemoryAssoc()
    _cache(assoc, nodes, [ix["intern"], ix["extern"]])
    w, ran, resolved = _evaluate(nodes, [ix["extern"]], assoc, nce=True)
    assert _executed(nodes, ran) == {ix["exec_a"], ix["exec_b"], ix["extern"]}
    assert resolved[ix["extern"]] == (W.READY, None) and w.looked_up == 0
    # without NoCacheExtern the same cache serves the extern
    nodes, ix = W.cache_lookup_bottomup_flow()
    w, ran, resolved = _evaluate(nodes, [ix["extern"]], assoc)
    assert resolved[ix["extern"]][0] == W.HIT and ix["extern"] not in ran


def test_consumer_of_an_extern_is_looked_up_bottom_up_only():
    """Eval.lookup never calls dirty; only top-down todo does (eval.go:908-913
    against :940-941, 1173)."""
    nodes, ix = P.no_cache_extern_flow()
    roots = [ix["top"], ix["clean_root"]]
    assoc = O.InmemoryAssoc()
    _cache(assoc, nodes, range(len(nodes)))
    plan = P.plan(nodes, roots, assoc, KIND, no_cache_extern=True)
    assert plan.states[ix["consumer"]] == P.TODO and ix["consumer"] not in plan.hits  # dirty: not looked up
    w, ran, resolved = _evaluate(nodes, roots, assoc, nce=True)
    assert resolved[ix["consumer"]][0] == W.HIT                  # looked up once its deps were done
    assert resolved[ix["clean"]][0] == W.HIT
    assert resolved[ix["extern"]] == (W.READY, None)             # an extern
    assert resolved[ix["top"]] == (W.READY, None)                # a listed root
    assert resolved[ix["clean_root"]] == (W.READY, None)
    assert w.states[ix["mapexec"]] == W.UNSEEN                   # Deps only: the MapFlow is not walked


@pytest.mark.parametrize("flow", ["cache_lookup", "no_cache_extern", "random"])
def test_begin_states_takes_over_a_plan(flow):
    if flow == "cache_lookup":
        nodes, ix = P.cache_lookup_flow()
        roots, nce, cached = [ix["extern"]], False, [ix["intern"]]
    elif flow == "no_cache_extern":
        nodes, ix = P.no_cache_extern_flow()
        roots, nce, cached = [ix["top"], ix["clean_root"]], True, range(len(nodes))
    else:
        case = C.Case(2, 200, False)
        nodes, roots, nce, cached = case.nodes, case.roots, False, range(0, len(case.nodes), 3)
    assoc = O.InmemoryAssoc()
    _cache(assoc, nodes, cached)
    plan = P.plan(nodes, roots, assoc, KIND, node_keys=P.cache_keys_of(nodes), no_cache_extern=nce)
    w = W.Wave(nodes)
    w.begin_states(plan.states)
    assert w.list(W.READY, W.LAST)[0].tolist() == plan.list(P.READY)[0].tolist() == w.history[0]
    assert w.list(W.READY)[0].tolist() == plan.list(P.READY)[0].tolist()
    assert w.list(W.TODO)[0].tolist() == plan.list(P.TODO)[0].tolist()
    assert w.list(W.UNSEEN)[0].tolist() == plan.list(P.UNSEEN)[0].tolist()
    assert w.counts()[W.DONE] == plan.counts()[P.HIT] + plan.counts()[P.DONE] and w.counts()[W.HIT] == 0
    while w.last:  # to the end: nothing is ever looked up (eval.go:943-947)
        w.step(w.list(W.READY, W.LAST)[0])
        assert w.looked_up == 0 and w.counts()[W.HIT] == 0
    assert w.counts()[W.TODO] == w.counts()[W.READY] == 0
    assert all(w.states[r] == W.DONE for r in roots)


def test_refusals_leave_the_model_unchanged():
    w = W.Wave(dep_lists=[[1, 2, 2], [3], [3], [], []], flags=[1, 1, 1, 1, 1])
    assoc = O.InmemoryAssoc()
    keys = [[C.fake_key(b"k", i)] for i in range(5)]
    assoc.put(KIND, None, keys[3][0], P.fileset_id(3))
    w.begin([0], assoc, KIND, keys)
    assert w.states.tolist() == [W.TODO, W.TODO, W.TODO, W.HIT, W.UNSEEN] and w.pending[0] == 3

    def snapshot():
        return w.states.tolist(), list(w.pending), sorted(w.last), w.waves
    before = snapshot()
    with pytest.raises(W.Refused):
        w.step([3, 1], assoc, KIND, keys)  # a TODO node
    with pytest.raises(W.Refused):
        w.reject([3, 0])
    with pytest.raises(W.Refused):
        w.begin_states([W.TODO, W.UNSEEN, W.DONE, W.DONE, 0])  # an UNSEEN dep under a TODO
    with pytest.raises(W.Refused):
        w.begin_states([W.DONE, W.DONE, W.DONE, W.DONE, 5])
    assert snapshot() == before
    w.step([3, 3], assoc, KIND, keys)  # listed twice: one decrement per consumer entry
    assert sorted(w.last) == [1, 2] and w.pending[0] == 3
    w.step([2], assoc, KIND, keys)  # the dep listed twice: two entries
    assert w.pending[0] == 1 and not w.last
    w.step([], assoc, KIND, keys)
    assert not w.last and w.waves == 4
    w.step([1], assoc, KIND, keys)
    assert sorted(w.last) == [0] and w.states[4] == W.UNSEEN


def test_absent_keys():
    w = W.Wave(dep_lists=[[]], flags=[1])
    assoc = O.InmemoryAssoc()
    logical = C.fake_key(b"logical", 0)
    assoc.put(KIND, None, logical, P.fileset_id(0))
    w.begin([0], assoc, KIND, [[W.ZERO, logical]])
    assert w.hits[0] == (1, P.fileset_id(0), 0b10) and w.keys_probed == 1 and w.looked_up == 1
    w.begin([0], assoc, KIND, [[W.ZERO, W.ZERO]])
    assert w.states[0] == W.READY and w.looked_up == 0 and w.keys_probed == 0


def test_scenarios_cover_the_cases():
    """What tests/test_gpu_wave.py's random flows exercise, asserted on the
    model alone: every state, a wave holding both HIT and READY, a rejected
    hit, a filtered key, a hit under its second key, hits in later waves."""
    total = {"states": set(), "which": set(), "mixed_wave": 0, "rejected": 0, "filtered": 0, "late_hits": 0}
    for seed, n, with_liveset in C.SEEDS:
        case = C.Case(seed, n, with_liveset)
        target = C.ModelTarget(case)
        seen = C.play(case, target)
        m = target.model
        flat = [i for wave in m.history for i in wave]
        assert len(flat) == len(set(flat))                     # each node in exactly one wave
        assert all(m.states[r] == W.DONE for r in case.roots)  # a complete evaluation
        assert m.counts()[W.TODO] == m.counts()[W.READY] == m.counts()[W.HIT] == 0
        assert seen["states"] == {0, 1, 2, 3, 4} and seen["steps"] >= 5, (seed, seen)
        assert (seen["filtered"] > 0) == with_liveset, (seed, seen)
        for k, v in seen.items():
            if k in total:
                total[k] = total[k] | v if isinstance(v, set) else total[k] + v
    assert total["which"] >= {0, 1} and total["mixed_wave"] > 0 and total["rejected"] > 0
    assert total["filtered"] > 0 and total["late_hits"] > 0
    # the seeds that carry the rest on their own, with and without a liveset
    for seed, n, with_liveset in [(2, 200, False), (3, 300, True)]:
        case = C.Case(seed, n, with_liveset)
        seen = C.play(case, C.ModelTarget(case))
        assert seen["which"] >= {0, 1} and seen["mixed_wave"] and seen["rejected"] and seen["late_hits"]
        assert any(case.invalid) and any(f.done for f in case.nodes)
        assert any(len([k for k in ks if k != W.ZERO]) == 2 for ks in case.keys())
