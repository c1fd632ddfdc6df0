"""CPU restatement of the GC liveset (rf_liveset_*): Eval.collect
(eval.go:791-868) over OFlow nodes (done, value, deps, mapflow).  A helper,
not a test.

  walk (eval.go:809-826): from the root, a node that is FlowDone with a
  Fileset value ends the walk there (:812-816); every other node is visited
  (:818) and, when it is an OpMap, its MapFlow is pushed too (:822-824).
  writers (:827-835): each writer's value follows the frontier's, in order.
  sizing (:813-814, :832, :838-843): nlive_est = the sum of Fileset.N()
  (executor.go:95-102: not unique); bloom.NewWithEstimates(nlive_est, 0.001)
  (bloom.go:81-83, 120-131) or bloom.New(64, 1).
  filter (:848-858): per value, Files() -- a map[File]bool, so the distinct
  (ID, Size) pairs of that value alone (executor.go:82-92, 116-125) -- each
  added as WD(ID); nlive counts them, livebytes sums their sizes.
  changed (:862): no previous filter, or !Equal (bloom.go:347-349: m, k and
  the bitset; bitset.go:322-340: length and every word).

Where the reference skips a value with N() == 0 (:813, :831) the model keeps it
as a contribution of zero rows, as rf_liveset counts it: it adds nothing to
any other figure.

Built on the oracle's pieces: estimate_parameters, orc_bloomlive_add_batch and
orc_bloomlive_contains_batch."""
from __future__ import annotations

import numpy as np

import reflow_oracle as O

UNSEEN, WALKED, VALUE = range(3)


def value_rows(fs):
    """The (ID, Size) rows of a Fileset: Map entries with List flattened
    recursively -- exactly Fileset.N() of them (executor.go:95-102)."""
    out = []
    for v in fs.list or []:
        out.extend(value_rows(v))
    out.extend((bytes(fid), int(size)) for fid, size in (fs.map or {}).values())
    return out


def has_value(f) -> bool:
    """State == FlowDone and Value is a Fileset (eval.go:810-812)."""
    return bool(f.done) and isinstance(f.value, O.OFileset)


def edges_of(f):
    """Deps, and for an OpMap its MapFlow (eval.go:818-824)."""
    out = list(f.deps)
    if f.op == O.OP["OpMap"] and f.mapflow is not None:
        out.append(f.mapflow)
    return out


def all_nodes(root):
    """Every node beneath root along the walk's edges, root first."""
    nodes, seen, stack = [], set(), [root]
    while stack:
        f = stack.pop()
        if id(f) in seen:
            continue
        seen.add(id(f))
        nodes.append(f)
        stack.extend(edges_of(f))
    return nodes


def live_csr(nodes):
    """(edge_ptr uint64 [n+1], edges uint32) as rf_liveset_open takes them."""
    idx = {id(f): i for i, f in enumerate(nodes)}
    ptr, edges = [0], []
    for f in nodes:
        edges.extend(idx[id(d)] for d in edges_of(f))
        ptr.append(len(edges))
    return np.array(ptr, np.uint64), np.array(edges, np.uint32)


def value_arrays(nodes, which=None):
    """(nodes uint32, counts uint32, ids uint8 [rows, 32], sizes int64) of the
    listed nodes that have a value (default: all), as rf_liveset_set_values
    takes them."""
    sel = range(len(nodes)) if which is None else which
    nd, ct, ids, sz = [], [], [], []
    for i in sel:
        if has_value(nodes[i]):
            rows = value_rows(nodes[i].value)
            nd.append(i)
            ct.append(len(rows))
            ids.extend(r[0] for r in rows)
            sz.extend(r[1] for r in rows)
    return (np.array(nd, np.uint32), np.array(ct, np.uint32),
            np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32).copy(), np.array(sz, np.int64))


class Live:
    def __init__(self, states, contributions, nlive_est, nlive, livebytes, m, k, words, length, changed):
        self.states = states                  # uint8 [n]
        self.contributions = contributions    # node per contribution: frontier ascending, then writers
        self.nlive_est, self.nlive, self.livebytes = nlive_est, nlive, livebytes
        self.m, self.k, self.words, self.length = m, k, words, length
        self.changed = changed

    def counts(self):
        return [int((self.states == s).sum()) for s in range(3)]

    def list(self, state):
        return np.flatnonzero(self.states == state).astype(np.uint32)

    def contains(self, ids) -> np.ndarray:
        """bloomlive Contains of each 32-byte id (bloomlive.go:30-36)."""
        ids = [bytes(i) for i in ids]
        out = np.zeros(max(len(ids), 1), dtype=np.uint8)
        if ids:
            O.lib().orc_bloomlive_contains_batch(self.words.ctypes.data, self.length, self.m, self.k, b"".join(ids),
                                                 len(ids), out.ctypes.data, 1)
        return out[:len(ids)].astype(bool)

    def equal(self, other) -> bool:
        """BloomFilter.Equal (bloom.go:347-349, bitset.go:322-340)."""
        return (self.m == other.m and self.k == other.k and self.length == other.length
                and np.array_equal(self.words, other.words))


def live(nodes, roots, writers=(), prev=None):
    """nodes: OFlow list (Deps and MapFlows among them); roots, writers:
    indices; prev: the previous collection's Live or None."""
    idx = {id(f): i for i, f in enumerate(nodes)}
    states = np.zeros(len(nodes), dtype=np.uint8)
    stack = [int(r) for r in roots]
    while stack:  # eval.go:809-826
        i = stack.pop()
        if states[i] != UNSEEN:
            continue
        if has_value(nodes[i]):
            states[i] = VALUE
            continue
        states[i] = WALKED
        stack.extend(idx[id(d)] for d in edges_of(nodes[i]))
    contributions = [int(i) for i in np.flatnonzero(states == VALUE)] + [int(w) for w in writers]  # :827-835
    livevals = [value_rows(nodes[i].value) if has_value(nodes[i]) else [] for i in contributions]
    nlive_est = sum(len(v) for v in livevals)  # :813-814, :832
    if nlive_est > 0:  # :838-843
        m, k = O.estimate_parameters(nlive_est, 0.001)
        m, k = max(1, m), max(1, k)  # bloom.New (bloom.go:81-83)
    else:
        m, k = 64, 1
    words = np.zeros((m + 63) // 64, dtype=np.uint64)
    length = np.array([m], dtype=np.uint64)  # bitset.New(m)
    nlive, livebytes = 0, 0
    for v in livevals:  # :848-858
        files = set(v)  # Files(): map[File]bool of this value alone
        nlive += len(files)
        livebytes += sum(size for _, size in files)
    keys = [fid for v in livevals for fid, _ in v]
    if keys:
        O.lib().orc_bloomlive_add_batch(words.ctypes.data, length.ctypes.data, m, k, b"".join(keys), len(keys))
    out = Live(states, contributions, nlive_est, nlive, livebytes, m, k, words, int(length[0]), True)
    out.changed = prev is None or not prev.equal(out)  # :862
    return out


def files(*specs):
    """testutil.Files("path:contents", ...): path -> (sha256(contents), len(contents))."""
    out = {}
    for s in specs:
        path, contents = s.split(":")
        out[path] = (O.sha256(contents.encode()), len(contents))
    return O.OFileset(map=out)


GC_FILES = ["a/x:x", "a/y:y", "a/z:z", "b/1:1", "b/2:2", "c/xxx:xxx", "orphan:orphan", "unrooted:unrooted"]
GC_EXPECT = ["x:x", "y:y", "z:z", "1:1", "2:2", "xxx:xxx", "anotherfile:orphan"]


def gc_flow():
    """TestGC's flow (test/evaltest/eval_test.go:353-362) as a static graph:
    pullup(map(map(groupby(intern)))); the second map's function closes over
    collect("orphan", intern).  Returns (nodes, name -> index); the root is
    "pullup".  Nothing is done yet: gc_stage sets the values."""
    intern = O.OFlow("OpIntern", url="internurl")
    groupby = O.OFlow("OpGroupby", [intern], re="^(.)/.*")
    arg1 = O.OFlow("OpVal", flow_digest=O.from_string("arg1"))
    map_collect = O.OFlow("OpMap", [groupby], mapflow=O.OFlow("OpCollect", [arg1], re="^./(.*)", repl="$1"))
    orphan = O.OFlow("OpCollect", [intern], re="orphan", repl="anotherfile")
    arg2 = O.OFlow("OpVal", flow_digest=O.from_string("arg2"))
    map_pullup = O.OFlow("OpMap", [map_collect], mapflow=O.OFlow("OpPullup", [arg2, orphan]))
    pullup = O.OFlow("OpPullup", [map_pullup])
    nodes = all_nodes(pullup)
    name = dict(intern=intern, groupby=groupby, map_collect=map_collect, orphan=orphan, map_pullup=map_pullup,
                pullup=pullup)
    return nodes, {k: next(i for i, f in enumerate(nodes) if f is v) for k, v in name.items()}


def gc_stage(nodes, ix, stage):
    """TestGC's evaluation at 0: nothing done; 1: the intern done (:382);
    2: intern and groupby done; 3: the root done with its seven files (:387)."""
    for f in nodes:
        f.done, f.value = False, None
    if stage >= 1:
        nodes[ix["intern"]].done, nodes[ix["intern"]].value = True, files(*GC_FILES)
    if stage >= 2:
        groups = [files("a/x:x", "a/y:y", "a/z:z"), files("b/1:1", "b/2:2"), files("c/xxx:xxx")]
        nodes[ix["groupby"]].done, nodes[ix["groupby"]].value = True, O.OFileset(list=groups)
    if stage >= 3:
        nodes[ix["pullup"]].done, nodes[ix["pullup"]].value = True, files(*GC_EXPECT)


def gc_objects():
    """The eight objects TestGC puts into the repository (:372-381): (ids [8, 32], sizes)."""
    contents = [s.split(":")[1].encode() for s in GC_FILES]
    ids = np.frombuffer(b"".join(O.sha256(c) for c in contents), np.uint8).reshape(-1, 32).copy()
    return ids, np.array([len(c) for c in contents], np.int64)
