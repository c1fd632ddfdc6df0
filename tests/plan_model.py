"""CPU restatement of the evaluation plan (rf_eval_plan_*): Eval.todo and
Eval.lookup in top-down mode (eval.go:902-955, 1163-1269) over OFlow nodes.
A helper, not a test.

  todo (eval.go:902-955): from the root, a FlowInit node that is OpIntern,
  OpExec or OpExtern and not dirty (:908-913; Eval.dirty :874-887, only under
  NoCacheExtern) is looked up; every other node is FlowTODO at once and its
  Deps are visited (:915-920).  A FlowDone node is left alone.
  lookup (eval.go:1172-1269): fails at once for an invalidated node, for an
  OpExtern or the root under NoCacheExtern (:1173) and for a node without keys
  (:1183-1188); otherwise the keys are tried in CacheKeys order (flow.go:796-802)
  and the first one with a value wins (:1202-1220).  A failed lookup makes the
  node FlowTODO in top-down mode (:1163-1169) and todo goes on beneath it.
  A liveset filters keys before the assoc (a key it does not contain counts as
  NotExist).  A TODO node whose Deps are all done -- FlowDone already, or a
  cache hit (:1262) -- is what todo makes FlowNeedTransfer / FlowReady
  (:930-953): READY.

Built on the oracle's pieces: reflow_oracle.eval_dirty, InmemoryAssoc,
assoc_lookup and the bloomlive Contains (orc_bloomlive_contains_batch)."""
from __future__ import annotations

import numpy as np

import reflow_oracle as O

F_CACHEABLE, F_EXTERN, F_INVALID, F_DONE = 1, 2, 4, 8
UNSEEN, TODO, READY, HIT, DONE = range(5)
_CACHEABLE_OPS = (O.OP["OpIntern"], O.OP["OpExec"], O.OP["OpExtern"])


class Liveset:
    """A bloomlive filter built by the oracle (bloom.go:182-190 over WD(d))."""

    def __init__(self, keys, p=0.01):
        n = max(len(keys), 1)
        self.m, self.k = O.estimate_parameters(n, p)
        self.words = np.zeros((self.m + 63) // 64, dtype=np.uint64)
        length = np.array([self.m], dtype=np.uint64)
        if keys:
            O.lib().orc_bloomlive_add_batch(self.words.ctypes.data, length.ctypes.data, self.m, self.k,
                                            b"".join(keys), len(keys))
        self.length = int(length[0])

    def contains(self, key: bytes) -> bool:
        out = np.zeros(1, dtype=np.uint8)
        O.lib().orc_bloomlive_contains_batch(self.words.ctypes.data, self.length, self.m, self.k, key, 1,
                                             out.ctypes.data, 1)
        return bool(out[0])


class _Filtered:
    """The assoc behind a liveset: Get of a key the liveset rules out is NotExist."""

    def __init__(self, assoc, live):
        self.assoc, self.live = assoc, live

    def get(self, kind, k):
        if self.live is not None and not self.live.contains(k):
            return None
        return self.assoc.get(kind, k)


def flow_flags(nodes, invalid=()):
    inv = set(invalid)
    out = np.zeros(len(nodes), dtype=np.uint8)
    for i, f in enumerate(nodes):
        out[i] = ((F_CACHEABLE if f.op in _CACHEABLE_OPS else 0) | (F_EXTERN if f.op == O.OP["OpExtern"] else 0) |
                  (F_INVALID if i in inv else 0) | (F_DONE if f.done else 0))
    return out


def flow_csr(nodes):
    """(dep_ptr uint64 [n+1], deps uint32): node i's Deps, as rf_flow_dirty takes them."""
    idx = {id(f): i for i, f in enumerate(nodes)}
    ptr, deps = [0], []
    for f in nodes:
        deps.extend(idx[id(d)] for d in f.deps)
        ptr.append(len(deps))
    return np.array(ptr, np.uint64), np.array(deps, np.uint32)


def key_arrays(node_keys):
    """(key_ptr uint64 [n+1], keys uint8 [K, 32]) of per-node key lists."""
    ptr = np.zeros(len(node_keys) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(k) for k in node_keys])
    flat = b"".join(k for ks in node_keys for k in ks)
    return ptr, np.frombuffer(flat, dtype=np.uint8).reshape(-1, 32).copy()


class Plan:
    def __init__(self, states, hits):
        self.states = states      # uint8 [n]
        self.hits = hits          # node -> (which, value, found mask)

    def counts(self):
        return [int((self.states == s).sum()) for s in range(5)]

    def list(self, state):
        """What rf_eval_plan_list gives: nodes ascending; for HIT also which,
        values and found masks (zero-length arrays otherwise)."""
        nodes = np.flatnonzero(self.states == state).astype(np.uint32)
        if state != HIT:
            return nodes, None, None, None
        which = np.array([self.hits[int(i)][0] for i in nodes], dtype=np.uint8)
        vals = np.frombuffer(b"".join(self.hits[int(i)][1] for i in nodes), dtype=np.uint8).reshape(-1, 32)
        mask = np.array([self.hits[int(i)][2] for i in nodes], dtype=np.uint8)
        return nodes, which, vals, mask


def plan(nodes, roots, assoc, kind, node_keys=None, live=None, no_cache_extern=False, invalid=()):
    """nodes: OFlow list (Deps among them); roots: indices; assoc: an
    InmemoryAssoc; node_keys: per node its cache keys (default
    f.cache_keys()); live: a Liveset or None; invalid: the indices
    Eval.Invalidate names."""
    n = len(nodes)
    idx = {id(f): i for i, f in enumerate(nodes)}
    if node_keys is None:
        node_keys = [f.cache_keys() for f in nodes]
    inv, root_set = set(invalid), set(int(r) for r in roots)
    table = _Filtered(assoc, live)
    memo = {}
    states = np.zeros(n, dtype=np.uint8)
    hits = {}
    reached = set()
    stack = [int(r) for r in roots]
    while stack:
        i = stack.pop()
        if i in reached:
            continue
        reached.add(i)
        f = nodes[i]
        if f.done:  # todo leaves a FlowDone node alone (eval.go:906-907: no case for it)
            states[i] = DONE
            continue
        look = (f.op in _CACHEABLE_OPS and not O.eval_dirty(f, no_cache_extern, memo)  # eval.go:908-913
                and i not in inv                                                      # :1173 valid
                and not (no_cache_extern and (f.op == O.OP["OpExtern"] or i in root_set))  # :1173
                and len(node_keys[i]) > 0)                                            # :1183-1188
        if look:
            which, val, got = O.assoc_lookup(table, kind, [node_keys[i]])[0]
            if which >= 0:
                states[i] = HIT
                hits[i] = (which, val, sum(1 << j for j, v in enumerate(got) if v is not None))
                continue
        states[i] = TODO  # lookupFailed, top-down (eval.go:1163-1169), or not looked up (:915)
        stack.extend(idx[id(d)] for d in f.deps)
    ready = [i for i in range(n)
             if states[i] == TODO and all(states[idx[id(d)]] in (HIT, DONE) for d in nodes[i].deps)]
    states[ready] = READY
    return Plan(states, hits)


def reject(nodes, roots, assoc, kind, rejected, invalid=(), **kw):
    """rf_eval_plan_reject restated: with the assoc and liveset unchanged, a
    fresh run with the rejected hits invalid (their lookups fail, :1268)."""
    return plan(nodes, roots, assoc, kind, invalid=set(invalid) | set(int(r) for r in rejected), **kw)


def all_nodes(root):
    """Every node beneath root -- Deps, MapFlow and Parent -- root first."""
    seen, out, stack = set(), [], [root]
    while stack:
        f = stack.pop()
        if id(f) in seen:
            continue
        seen.add(id(f))
        out.append(f)
        stack.extend(f.deps)
        if f.mapflow is not None:
            stack.append(f.mapflow)
        if f.parent is not None:
            stack.append(f.parent)
    return out


def cache_lookup_flow():
    """TestCacheLookup's flow (test/evaltest/eval_test.go:174-183):
    extern(pullup(map(groupby(intern)))), the map function an exec.  Returns
    (nodes, name -> index); the root is "extern"."""
    intern = O.OFlow("OpIntern", url="internurl")
    groupby = O.OFlow("OpGroupby", [intern], re="(.*)")
    mapexec = O.OFlow("OpExec", [O.OFlow("OpVal", value=O.OFileset(map={}))], image="image", cmd="command")
    mp = O.OFlow("OpMap", [groupby], mapflow=mapexec)
    pullup = O.OFlow("OpPullup", [mp])
    extern = O.OFlow("OpExtern", [pullup], url="externurl")
    nodes = all_nodes(extern)
    name = dict(intern=intern, groupby=groupby, mapexec=mapexec, map=mp, pullup=pullup, extern=extern)
    return nodes, {k: next(i for i, f in enumerate(nodes) if f is v) for k, v in name.items()}


def no_cache_extern_flow():
    """TestNoCacheExtern's flow (test/evaltest/eval_test.go:314-323) under a
    top exec, with an exec over the extern (dirty through its Dep), a clean exec
    over the intern, and a second clean exec that is listed as a root."""
    intern = O.OFlow("OpIntern", url="internurl")
    groupby = O.OFlow("OpGroupby", [intern], re="(.*)")
    mapexec = O.OFlow("OpExec", [O.OFlow("OpVal", value=O.OFileset(map={}))], image="image", cmd="command")
    mp = O.OFlow("OpMap", [groupby], mapflow=mapexec)
    pullup = O.OFlow("OpPullup", [mp])
    extern = O.OFlow("OpExtern", [pullup], url="externurl")
    consumer = O.OFlow("OpExec", [extern, intern], image="img", cmd="consume")
    clean = O.OFlow("OpExec", [intern], image="img", cmd="clean")
    top = O.OFlow("OpExec", [consumer, extern, clean], image="img", cmd="top")
    clean_root = O.OFlow("OpExec", [intern], image="img", cmd="clean root")
    nodes = all_nodes(O.OFlow("OpMerge", [top, clean_root]))[1:]
    name = dict(intern=intern, groupby=groupby, mapexec=mapexec, map=mp, pullup=pullup, extern=extern,
                consumer=consumer, clean=clean, top=top, clean_root=clean_root)
    return nodes, {k: next(i for i, f in enumerate(nodes) if f is v) for k, v in name.items()}


def fileset_id(i: int) -> bytes:
    """A nonzero stand-in for a Fileset id."""
    return O.sha256(b"fileset %d" % i)


def cache_keys_of(nodes):
    """[f.cache_keys() for f in nodes], with Flow.Digest memoized per node for
    the duration (it is sync.Once-memoized in the reference, flow.go:653-664;
    the oracle recomputes, which is exponential on a DAG with sharing)."""
    memo, orig = {}, O.OFlow.digest

    def digest(self, universe=b"", merged=False):
        k = (id(self), universe, merged)
        if k not in memo:
            memo[k] = orig(self, universe, merged)
        return memo[k]
    O.OFlow.digest = digest
    try:
        return [f.cache_keys() for f in nodes]
    finally:
        O.OFlow.digest = orig
