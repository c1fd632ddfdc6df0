"""CPU restatement of the cache write (rf_eval_wave_cache_write): Eval.CacheWrite
(eval.go:1113-1154) for a batch of finished nodes.  A helper, not a test.

  The assoc is a dict (kind, key) -> fsid and the repository a dict fsid ->
  size (test/testutil/assoc.go:16-56, test/testutil/repository.go:25-115).
  A listed node takes part iff it is OpIntern / OpExec / OpExtern (CACHEABLE),
  is not an OpExtern under NoCacheExtern (eval.go:1131) and has a present key;
  a key of 32 zero bytes is a PhysicalDigest that is not computable
  (flow.go:762-774), which CacheKeys omits (:798-800).  Whether Eval.Invalidate
  named the node does not matter for a write.  It then Puts its value's
  (fsid, JSON length) into the repository (marshal, eval.go:1961-1967; first
  size wins) and key -> fsid under every present key (eval.go:1146-1152); Puts
  apply in node order then key order, so of two writers of one key the later
  one stays.

play() is a bottom-up evaluation over a wave_cases.Case in which the fake
Put of what finished is this write: after every step, the nodes that RAN are
listed (one of them twice) with their values.  tests/test_cwrite_model.py
asserts what the chosen seeds cover; tests/test_gpu_cache_write.py replays
them on the device."""
from __future__ import annotations

import random

import plan_model as P
import reflow_oracle as O
import wave_cases as C
import wave_model as W

KIND = C.KIND
WRITTEN, NOT_CACHEABLE, EXTERN, NO_KEY = range(4)
# (DAG seed, nodes, no_cache_extern): picked on the CPU from the model alone
SEEDS = [(1, 80, False), (2, 200, True), (6, 120, False), (40, 150, True)]


class Refused(ValueError):
    """What the library answers with RF_EINVAL; nothing has changed."""


def participation(flag, keys, no_cache_extern):
    """(reason, present keys) of one listed node."""
    if not flag & W.F_CACHEABLE:
        return NOT_CACHEABLE, []
    if no_cache_extern and flag & W.F_EXTERN:
        return EXTERN, []
    present = [k for k in keys if k != W.ZERO]
    return (WRITTEN if present else NO_KEY), present


class Tables:
    """The assoc and the repository index as dicts."""

    def __init__(self):
        self.assoc = {}  # (kind, key) -> fsid
        self.repo = {}   # fsid -> size

    def write(self, flags, states, node_keys, nodes, fsids, sizes, kind=KIND, no_cache_extern=False, repo=True):
        """One rf_eval_wave_cache_write.  Returns its rf_cache_write_out:
        (nodes written, keys put, [skipped by reason 1..3], keys put per listed node)."""
        if any(states[i] != W.DONE for i in nodes):
            raise Refused("a listed node is not DONE")
        skipped, per, written, puts = [0, 0, 0], [], 0, []
        for i, fsid, size in zip(nodes, fsids, sizes):
            reason, present = participation(int(flags[i]), node_keys[i], no_cache_extern)
            per.append(len(present))
            if reason != WRITTEN:
                skipped[reason - 1] += 1
                continue
            written += 1
            if repo:
                self.repo.setdefault(fsid, size)  # content addressing: the first size stays
            puts += [(k, fsid) for k in present]
        for k, v in puts:  # ops on one key apply in index order
            self.assoc[kind, k] = v
        return written, len(puts), skipped, per

    def assoc_entries(self, kind=KIND):
        return {k: v for (kd, k), v in self.assoc.items() if kd == kind}


class CwCase(C.Case):
    """A wave_cases.Case whose key rows also hold what a cache write has to
    get right: for a seeded tenth of the exec / extern nodes the physical row
    stays absent for good, a seeded eighth of the cacheable nodes has no present
    key at all, and seeded pairs of cacheable nodes share their logical key."""
    no_physical, no_key, alias = frozenset(), frozenset(), {}  # (Case.__init__ reads keys() before they are drawn)

    def __init__(self, seed, n, with_liveset=False):
        super().__init__(seed, n, with_liveset)
        rng = random.Random(77 * seed + n)
        two = [i for i, f in enumerate(self.nodes) if f.op in (O.OP["OpExec"], O.OP["OpExtern"])]
        self.no_physical = set(rng.sample(two, max(1, len(two) // 10)))
        cacheable = [i for i in range(len(self.nodes)) if P.flow_flags([self.nodes[i]])[0] & P.F_CACHEABLE]
        rng.shuffle(cacheable)
        self.no_key = set(cacheable[-max(1, len(cacheable) // 8):])
        self.alias = {b: a for a, b in zip(cacheable[0::2], cacheable[1::2]) if rng.random() < 0.3}
        leaves = [i for i in cacheable if not self.nodes[i].deps and not self.nodes[i].done]  # wave 0 together
        self.alias.update({b: a for a, b in zip(leaves[0::2], leaves[1::2])})
        self.puts, self.other, self.deleted = [], [], []  # the cache starts empty: every entry comes from a write

    def keys(self):
        out = super().keys()
        for i in self.no_physical:
            out[i][0] = W.ZERO
        for b, a in self.alias.items():
            out[b][-1] = out[a][-1]
        for i in self.no_key:
            out[i] = [W.ZERO] * len(out[i])
        return out


def value_of(i):
    """Node i's output: a few files, nested for every third node."""
    v = W.files(*("out%d/%d" % (i, j) for j in range(i % 4)))
    return O.OFileset(list=[v, W.files("x")]) if i % 3 == 0 else v


class ModelTarget:
    """play()'s calls on the model alone."""

    def __init__(self, case):
        self.ref = O.InmemoryAssoc()  # what the wave model looks up: kept equal to tables.assoc
        self.tables = Tables()
        self.model = W.Wave(case.nodes, case.invalid)
        self.outs = []

    def begin(self, roots, keys, no_cache_extern):
        self.model.begin(roots, self.ref, KIND, keys, no_cache_extern=no_cache_extern)

    def step(self, finished, keys):
        self.model.step(finished, self.ref, KIND, keys)

    def write(self, listed, values, keys, no_cache_extern):
        jsons = [v.json() for v in values]
        out = self.tables.write(self.model.flags, self.model.states, keys, listed, [O.sha256(j) for j in jsons],
                                [len(j) for j in jsons], no_cache_extern=no_cache_extern)
        self.ref.m = dict(self.tables.assoc)
        self.outs.append(out)
        return out

    def check(self):
        pass


def play(case, target, no_cache_extern=False):
    """A bottom-up evaluation of `case` with cache writes.  Returns what
    happened: reasons seen, whether a participating node had an absent
    physical key, whether two nodes of one batch shared a key, batches, late
    hits (nodes served by an entry a write of this run made)."""
    rng, nodes, m = case.rng, case.nodes, target.model
    seen = {"reasons": set(), "absent_physical": 0, "shared_key": 0, "twice": 0, "batches": 0, "late_hits": 0,
            "ran": [], "accepted": []}
    target.begin(case.roots, case.keys(), no_cache_extern)
    target.check()
    while True:
        open_ = [int(i) for i in list(m.list(W.READY)[0]) + list(m.list(W.HIT)[0])]
        if not open_:
            break
        done = [i for i in open_ if rng.random() < 0.6] or open_[:1]
        ran = [i for i in done if m.states[i] == W.READY]
        seen["accepted"] += [i for i in done if m.states[i] == W.HIT]
        seen["late_hits"] += sum(1 for i in done if m.states[i] == W.HIT)
        seen["ran"] += ran
        for i in done:
            nodes[i].done = True
            if i in ran or nodes[i].value is None:
                nodes[i].value = value_of(i)
        after = case.keys()
        target.step(done, after)
        target.check()
        listed = list(ran)
        rng.shuffle(listed)
        listed += listed[:1]  # (one of them listed twice)
        flags = m.flags
        batch_keys = {}
        for i in listed:
            reason, present = participation(int(flags[i]), after[i], no_cache_extern)
            seen["reasons"].add(reason)
            if reason == WRITTEN:
                seen["absent_physical"] += len(after[i]) == 2 and after[i][0] == W.ZERO
                for k in present:
                    seen["shared_key"] += any(j != i for j in batch_keys.get(k, ()))
                    batch_keys.setdefault(k, set()).add(i)
        seen["twice"] += len(listed) > len(set(listed))
        target.write(listed, [nodes[i].value for i in listed], after, no_cache_extern)
        seen["batches"] += 1
        target.check()
    return seen
