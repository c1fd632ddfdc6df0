"""CPU restatement of the evaluation waves (rf_eval_wave_*): Eval.todo and
Eval.lookup in bottom-up mode, and the completion step of either mode
(eval.go:902-955, 1163-1269, Deps only) over OFlow nodes.  A helper, not a
test.

  todo, bottom-up (eval.go:902-955): from the root every FlowInit node becomes
  FlowTODO without a lookup (:910 `!e.BottomUp`) and its Deps are visited; a
  FlowDone node is left alone.  A TODO node whose Deps are all done is looked
  up (:940-941) and, when that fails, becomes FlowNeedTransfer (:1163-1166):
  READY here.  In top-down mode such a node goes to NeedTransfer at once
  (:943-947).
  lookup (eval.go:1172-1269): fails at once for an invalidated node, for an
  OpExtern or the root under NoCacheExtern (:1173) and for a node without keys
  (:1183-1188); Eval.dirty is not consulted (only top-down todo calls it).  The
  keys are tried in CacheKeys order and the first one with a value wins.  A
  key of 32 zero bytes stands for a PhysicalDigest that is not computable
  (flow.go:762-774), which CacheKeys omits (:798-800): absent, not probed.
  The reference re-walks the graph from the roots on every scheduling step;
  here a node carries `pending`, the number of its dep entries whose dep has
  not finished, and step() walks from the finished nodes to their consumers.

Built on the oracle's pieces: InmemoryAssoc, assoc_lookup and the bloomlive
Contains (plan_model.Liveset over orc_bloomlive_contains_batch)."""
from __future__ import annotations

import numpy as np

import plan_model as P
import reflow_oracle as O

F_CACHEABLE, F_EXTERN, F_INVALID, F_DONE = 1, 2, 4, 8
UNSEEN, TODO, READY, HIT, DONE = range(5)
ALL, LAST = 0, 1
NONE, BOTTOMUP, TOPDOWN = 0, 1, 2
ZERO = bytes(32)


def consumers(dep_lists):
    """rf_eval_wave_consumers, naively: for node d the nodes that list d, one
    entry per dep entry, ascending."""
    cons = [[] for _ in dep_lists]
    for i, dl in enumerate(dep_lists):
        for d in dl:
            cons[d].append(i)
    return cons


def wave_keys(nodes):
    """Per node the key rows a wave object is opened with: [physical, logical]
    for the ops that have a physical digest (OpExec, OpExtern; the physical row
    is zeros while it is not computable), [logical] otherwise."""
    memo, orig = {}, O.OFlow.digest

    def digest(self, universe=b"", merged=False):
        k = (id(self), universe, merged)
        if k not in memo:
            memo[k] = orig(self, universe, merged)
        return memo[k]
    O.OFlow.digest = digest
    try:
        out = []
        for f in nodes:
            if f.op in (O.OP["OpExec"], O.OP["OpExtern"]):
                out.append([f.physical_digest() or ZERO, f.digest()])
            else:
                out.append([f.digest()])
        return out
    finally:
        O.OFlow.digest = orig


class Refused(ValueError):
    """What the library answers with RF_EINVAL; the model is unchanged."""


class Wave:
    def __init__(self, nodes=None, invalid=(), dep_lists=None, flags=None):
        """nodes: OFlow list (Deps among them), flags from their ops, f.done and
        `invalid`; or dep_lists (index lists) and flags (RF_PLAN_F_* bytes)."""
        if nodes is not None:
            idx = {id(f): i for i, f in enumerate(nodes)}
            dep_lists = [[idx[id(d)] for d in f.deps] for f in nodes]
            flags = P.flow_flags(nodes, invalid)
        self.deps = [list(map(int, d)) for d in dep_lists]
        self.cons = consumers(self.deps)
        self.flags = np.array(flags, dtype=np.uint8)
        self.n = len(self.deps)
        self.mode = NONE
        self.states = np.zeros(self.n, dtype=np.uint8)
        self.pending = [0] * self.n
        self.hits = {}
        self.last = set()
        self.roots = set()
        self.nce = False
        self.waves = 0
        self.history = []  # per begin / step, the sorted members of its wave
        self.looked_up = self.keys_probed = self.keys_filtered = 0

    def set_flags(self, nodes, flags):
        for i, f in zip(nodes, flags):
            self.flags[int(i)] = f

    # ---- results
    def counts(self):
        return [int((self.states == s).sum()) for s in range(5)]

    def list(self, state, scope=ALL):
        """What rf_eval_wave_list gives: nodes ascending; for HIT also which,
        values and found masks."""
        nodes = [int(i) for i in np.flatnonzero(self.states == state) if scope == ALL or int(i) in self.last]
        nodes = np.array(nodes, dtype=np.uint32)
        if state != HIT:
            return nodes, None, None, None
        which = np.array([self.hits[int(i)][0] for i in nodes], dtype=np.uint8)
        vals = np.frombuffer(b"".join(self.hits[int(i)][1] for i in nodes), dtype=np.uint8).reshape(-1, 32)
        mask = np.array([self.hits[int(i)][2] for i in nodes], dtype=np.uint8)
        return nodes, which, vals, mask

    # ---- a wave resolved
    def _resolve(self, wave, assoc, kind, node_keys, live):
        self.last = set(wave)
        self.history.append(sorted(wave))
        self.waves += 1
        self.looked_up = self.keys_probed = self.keys_filtered = 0
        for i in sorted(wave):
            self.states[i] = READY
            if self.mode != BOTTOMUP:
                continue  # eval.go:943-947: no lookup
            f = int(self.flags[i])
            keys = node_keys[i]
            present = [j for j, k in enumerate(keys) if k != ZERO]
            look = bool(f & F_CACHEABLE) and not f & F_INVALID and len(present) > 0
            if look and self.nce:
                look = not (f & F_EXTERN or i in self.roots)  # eval.go:1173
            if not look:
                continue
            self.looked_up += 1
            probe = []
            for j in present:
                if live is not None and not live.contains(keys[j]):
                    self.keys_filtered += 1
                else:
                    probe.append(j)
            self.keys_probed += len(probe)
            which, val, got = O.assoc_lookup(assoc, kind, [[keys[j] for j in probe]])[0]
            if which >= 0:
                self.states[i] = HIT
                self.hits[i] = (probe[which], val, sum(1 << probe[j] for j, v in enumerate(got) if v is not None))

    # ---- begin
    def begin(self, roots, assoc, kind, node_keys, live=None, no_cache_extern=False):
        self.mode, self.nce = BOTTOMUP, bool(no_cache_extern)
        self.roots = set(int(r) for r in roots)
        self.states[:] = UNSEEN
        self.hits, self.waves, self.history = {}, 0, []
        reached, stack, wave = set(), [int(r) for r in roots], []
        while stack:
            i = stack.pop()
            if i in reached:
                continue
            reached.add(i)
            if self.flags[i] & F_DONE:  # left alone (eval.go:906-907), a satisfied dep
                self.states[i] = DONE
                continue
            self.states[i] = TODO
            self.pending[i] = sum(1 for d in self.deps[i] if not self.flags[d] & F_DONE)
            if self.pending[i] == 0:
                wave.append(i)
            stack.extend(self.deps[i])
        self._resolve(wave, assoc, kind, node_keys, live)

    def begin_states(self, states):
        st = np.array(states, dtype=np.uint8)
        assert len(st) == self.n
        tracked = (st == TODO) | (st == READY)
        if (st > DONE).any():
            raise Refused("a state byte above DONE")
        for i in np.flatnonzero(tracked):
            if any(st[d] == UNSEEN for d in self.deps[int(i)]):
                raise Refused("a tracked node over an UNSEEN dep")
        self.mode, self.nce, self.roots = TOPDOWN, False, set()
        self.hits, self.waves, self.history = {}, 0, []
        self.states[:] = UNSEEN
        self.states[(st == HIT) | (st == DONE)] = DONE
        self.states[tracked] = TODO
        wave = []
        for i in np.flatnonzero(tracked):
            i = int(i)
            self.pending[i] = sum(1 for d in self.deps[i] if tracked[d])
            if self.pending[i] == 0:
                wave.append(i)
        self._resolve(wave, None, 0, None, None)

    # ---- step, reject
    def step(self, finished, assoc=None, kind=0, node_keys=None, live=None):
        assert self.mode != NONE
        fin = sorted(set(int(i) for i in finished))  # a node listed twice counts once
        if any(self.states[i] not in (READY, HIT) for i in fin):
            raise Refused("step lists a node that is neither READY nor a HIT")
        wave = []
        for i in fin:
            self.states[i] = DONE
        for i in fin:
            for c in self.cons[i]:
                if self.states[c] != TODO:
                    continue  # untracked
                self.pending[c] -= 1
                if self.pending[c] == 0:
                    wave.append(c)
        self._resolve(wave, assoc, kind, node_keys, live)

    def reject(self, nodes):
        nodes = [int(i) for i in nodes]
        if any(self.states[i] != HIT for i in nodes):
            raise Refused("reject lists a node that is not a hit")
        for i in nodes:
            self.states[i] = READY


def evaluate(w, accept, finish):
    """A complete evaluation after a begin: hits for which accept(i) is false
    are rejected, every READY node of the wave `runs`; finish(nodes) is called
    with what is about to be reported done (set values, Put cache entries) and
    returns step()'s arguments (assoc, kind, node_keys, live).  Returns the
    nodes that ran, in order."""
    ran = []
    while w.last:
        hits = [int(i) for i in w.list(HIT, LAST)[0]]
        bad = [i for i in hits if not accept(i)]
        if bad:
            w.reject(bad)
        ready = [int(i) for i in w.list(READY, LAST)[0]]
        ran.extend(ready)
        done = sorted(set(hits) | set(ready))
        w.step(done, *finish(done))
    return ran


# ---- the reference's bottom-up flows, reduced to static graphs ----------------------
def _named(root, name):
    nodes = P.all_nodes(root)
    return nodes, {k: next(i for i, f in enumerate(nodes) if f is v) for k, v in name.items()}


def files(*names):
    """testutil.Files: a Fileset of the named files, each holding its name."""
    return O.OFileset(map={n: (O.sha256(n.encode()), len(n)) for n in names})


def cache_lookup_bottomup_flow():
    """TestCacheLookupBottomup (test/evaltest/eval_test.go:232-277) and
    TestNoCacheExtern (:314-351) after the Map has expanded over the groupby's
    two groups: extern(pullup(merge(groupby(intern), exec(a), exec(b)))), the
    execs over the values "a" and "b"."""
    intern = O.OFlow("OpIntern", url="internurl")
    groupby = O.OFlow("OpGroupby", [intern], re="(.*)")
    val_a = O.OFlow("OpVal", value=files("a"), done=True)
    val_b = O.OFlow("OpVal", value=files("b"), done=True)
    exec_a = O.OFlow("OpExec", [val_a], image="image", cmd="command")
    exec_b = O.OFlow("OpExec", [val_b], image="image", cmd="command")
    mapped = O.OFlow("OpMerge", [groupby, exec_a, exec_b])
    pullup = O.OFlow("OpPullup", [mapped])
    extern = O.OFlow("OpExtern", [pullup], url="externurl")
    return _named(extern, dict(intern=intern, groupby=groupby, val_a=val_a, val_b=val_b, exec_a=exec_a,
                               exec_b=exec_b, mapped=mapped, pullup=pullup, extern=extern))


def cache_lookup_missing_flow():
    """TestCacheLookupMissing (test/evaltest/eval_test.go:279-312): exec(intern)."""
    intern = O.OFlow("OpIntern", url="internurl")
    ex = O.OFlow("OpExec", [intern], image="image", cmd="command")
    return _named(ex, dict(intern=intern, exec=ex))
