"""The GC liveset's CPU model (tests/live_model.py) against the reference's
own behavioural test of garbage collection (test/evaltest/eval_test.go TestGC
:353-409) and the counting rules of Eval.collect (eval.go:791-868)."""
import numpy as np

import reflow_oracle as O

import live_model as M


def _ids(*contents):
    return [O.sha256(c.encode()) for c in contents]


def test_gc_intern_done():
    """Only the intern is done (:382): its eight files are the live set --
    `unrooted` included, nothing has superseded the intern's value yet."""
    nodes, ix = M.gc_flow()
    M.gc_stage(nodes, ix, 1)
    r = M.live(nodes, [ix["pullup"]])
    assert r.states[ix["intern"]] == M.VALUE
    assert all(r.states[i] == M.WALKED for i in range(len(nodes)) if i != ix["intern"])
    assert r.contributions == [ix["intern"]]
    assert (r.nlive_est, r.nlive, r.livebytes) == (8, 8, sum(len(s.split(":")[1]) for s in M.GC_FILES))
    assert (r.m, r.k, r.length) == (116, 11, 116)
    ids, _ = M.gc_objects()
    assert r.contains(ids).all()
    assert r.changed


def test_gc_root_done():
    """The root is done with its seven files (:387): they are live (:391-399)
    and `unrooted` is not (:400-408); nothing beneath the root is reached."""
    nodes, ix = M.gc_flow()
    M.gc_stage(nodes, ix, 3)
    r = M.live(nodes, [ix["pullup"]])
    assert r.states[ix["pullup"]] == M.VALUE
    assert r.counts() == [len(nodes) - 1, 0, 1]
    assert (r.nlive_est, r.nlive) == (7, 7)
    assert (r.m, r.k, r.length) == (101, 11, 101)
    assert r.contains(_ids("x", "y", "z", "1", "2", "xxx", "orphan")).all()
    assert not r.contains(_ids("unrooted"))[0]
    ids, _ = M.gc_objects()
    assert list(np.flatnonzero(~r.contains(ids))) == [7]  # what Repository.Collect removes


def test_gc_stages_change():
    nodes, ix = M.gc_flow()
    prev = None
    for stage in range(4):
        M.gc_stage(nodes, ix, stage)
        r = M.live(nodes, [ix["pullup"]], prev=prev)
        assert r.changed, stage
        again = M.live(nodes, [ix["pullup"]], prev=r)
        assert not again.changed and again.equal(r)
        prev = r
    M.gc_stage(nodes, ix, 0)
    r = M.live(nodes, [ix["pullup"]])
    assert (r.m, r.k, r.length, r.nlive_est, r.nlive, r.livebytes) == (64, 1, 64, 0, 0, 0)  # eval.go:842
    assert not r.words.any() and r.counts() == [0, len(nodes), 0]


def _fs(*pairs):
    return O.OFileset(map={"p%d" % i: (O.sha256(b"%d" % c), s) for i, (c, s) in enumerate(pairs)})


def test_double_counting_rules():
    a = O.OFlow("OpExec", done=True, value=_fs((1, 10), (2, 20), (1, 10)))   # a file twice in one value
    b = O.OFlow("OpExec", done=True, value=_fs((1, 10), (1, 11)))            # shared with a; one ID, two sizes
    e = O.OFlow("OpExec", done=True, value=_fs())                            # zero rows: still a value
    below = O.OFlow("OpExec", done=True, value=_fs((9, 9)))
    e.deps = [below]
    w = O.OFlow("OpExec", done=True, value=_fs((3, 5)))                      # only a writer reaches it
    nv = O.OFlow("OpExec", done=True, value=None)                            # Done, no Fileset: expanded
    nv.deps = [b]
    root = O.OFlow("OpMerge", [a, nv, e, a])
    nodes = [root, a, b, e, below, w, nv]
    r = M.live(nodes, [0, 0], writers=[5, 1, 5, 6])
    assert list(r.states) == [M.WALKED, M.VALUE, M.VALUE, M.VALUE, M.UNSEEN, M.UNSEEN, M.WALKED]
    assert r.contributions == [1, 2, 3, 5, 1, 5, 6]
    # N(): 3 + 2 + 0, then the writers 1 + 3 + 1 + 0
    assert r.nlive_est == 10
    # Files() per contribution: a 2, b 2, e 0, w 1, a 2, w 1, nv 0
    assert r.nlive == 8
    assert r.livebytes == (10 + 20) + (10 + 11) + 0 + 5 + (10 + 20) + 5
    assert (r.m, r.k) == O.estimate_parameters(10, 0.001)
    assert r.contains([O.sha256(b"%d" % c) for c in (1, 2, 3)]).all()


def test_list_and_map_rows():
    inner = O.OFileset(list=[_fs((1, 1)), O.OFileset(list=[_fs((2, 2), (3, 3))])], map={"m": (O.sha256(b"4"), 4)})
    assert sorted(s for _, s in M.value_rows(inner)) == [1, 2, 3, 4]
    f = O.OFlow("OpExec", done=True, value=inner)
    r = M.live([f], [0])
    assert (r.nlive_est, r.nlive, r.livebytes) == (4, 4, 10)
