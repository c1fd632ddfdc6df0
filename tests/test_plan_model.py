"""The evaluation plan's CPU model (tests/plan_model.py) against the
reference's own behavioural tests of top-down cache lookup
(test/evaltest/eval_test.go TestCacheLookup :174-230, TestNoCacheExtern
:314-351): which nodes are looked up, which hit, which are left to run."""
import reflow_oracle as O

import plan_model as M

KIND = 0  # assoc.Fileset


def _cached(nodes, which):
    a = O.InmemoryAssoc()
    for i in which:
        for k in nodes[i].cache_keys():
            a.put(KIND, None, k, M.fileset_id(i))
    return a


def test_cache_lookup_extern_cached():
    """WriteCache(extern.Digest()): no flow is executed (:195-203) -- only the
    extern is reached, and it is a hit."""
    nodes, ix = M.cache_lookup_flow()
    p = M.plan(nodes, [ix["extern"]], _cached(nodes, [ix["extern"]]), KIND)
    assert p.states[ix["extern"]] == M.HIT
    assert all(p.states[i] == M.UNSEEN for i in range(len(nodes)) if i != ix["extern"])
    assert p.hits[ix["extern"]] == (0, M.fileset_id(ix["extern"]), 1)  # its one key: no physical digest yet
    assert p.counts() == [len(nodes) - 1, 0, 0, 1, 0]


def test_cache_lookup_intern_cached():
    """WriteCache(intern.Digest()): the extern and the map's execs run
    (:214-229) -- extern, pullup, map and groupby are TODO, the intern is a hit,
    so groupby is ready; the map's exec is not a Dep and is never seen."""
    nodes, ix = M.cache_lookup_flow()
    p = M.plan(nodes, [ix["extern"]], _cached(nodes, [ix["intern"]]), KIND)
    assert [p.states[ix[k]] for k in ("extern", "pullup", "map")] == [M.TODO] * 3
    assert p.states[ix["groupby"]] == M.READY
    assert p.states[ix["intern"]] == M.HIT
    assert p.states[ix["mapexec"]] == M.UNSEEN
    nodes_hit, which, vals, mask = p.list(M.HIT)
    assert list(nodes_hit) == [ix["intern"]] and list(which) == [0] and list(mask) == [1]
    assert vals[0].tobytes() == M.fileset_id(ix["intern"])


def test_no_cache_extern():
    """NoCacheExtern with every key cached: the extern and the roots are never
    hits (eval.go:1173), an exec over the extern is dirty and not looked up
    (:910), a clean exec is a hit."""
    nodes, ix = M.no_cache_extern_flow()
    a = _cached(nodes, range(len(nodes)))
    roots = [ix["top"], ix["clean_root"]]
    p = M.plan(nodes, roots, a, KIND, no_cache_extern=True)
    for k in ("extern", "top", "clean_root", "consumer"):
        assert p.states[ix[k]] in (M.TODO, M.READY), k
    assert p.states[ix["clean"]] == M.HIT and p.states[ix["intern"]] == M.HIT
    assert p.states[ix["clean_root"]] == M.READY        # its one dep is a hit
    assert p.states[ix["consumer"]] == M.TODO           # waits for the extern
    assert p.states[ix["groupby"]] == M.READY
    # without NoCacheExtern the same cache answers at the roots
    q = M.plan(nodes, roots, a, KIND)
    assert q.states[ix["top"]] == M.HIT and q.states[ix["clean_root"]] == M.HIT
    assert q.counts()[M.HIT] == 2 and q.counts()[M.UNSEEN] == len(nodes) - 2


def test_reject_is_a_run_with_the_hits_invalid():
    nodes, ix = M.no_cache_extern_flow()
    a = _cached(nodes, range(len(nodes)))
    roots = [ix["top"]]
    p = M.reject(nodes, roots, a, KIND, [ix["top"]])
    assert p.states[ix["top"]] == M.READY  # consumer, extern and clean all hit
    assert [p.states[ix[k]] for k in ("consumer", "extern", "clean")] == [M.HIT] * 3
    assert p.states[ix["intern"]] == M.UNSEEN


def test_liveset_filters_before_the_assoc():
    nodes, ix = M.cache_lookup_flow()
    a = _cached(nodes, [ix["extern"], ix["intern"]])
    live = M.Liveset(nodes[ix["intern"]].cache_keys())  # the extern's key is not live
    p = M.plan(nodes, [ix["extern"]], a, KIND, live=live)
    assert p.states[ix["extern"]] == M.TODO and p.states[ix["intern"]] == M.HIT
