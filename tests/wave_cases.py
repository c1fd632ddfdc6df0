"""Seeded evaluation-wave scenarios over flowgen.random_dag flows, decided on
the CPU model alone (tests/wave_model.py) and replayed on anything that takes
the same calls.  A helper, not a test: tests/test_wave_model.py asserts what
the chosen seeds cover, tests/test_gpu_wave.py replays them on the device.

A scenario: a bottom-up begin from the nodes nobody depends on; then, until
nothing is left, a seeded share of the last wave's hits is rejected, a seeded
share of everything READY or HIT finishes (so completions are split across
steps), the finished nodes get values -- which makes their consumers'
physical keys computable -- and cache entries are Put between steps: the
finished nodes' own keys (CacheWrite) and some of the physical keys that have
just become computable, so later waves hit under key 0."""
from __future__ import annotations

import hashlib
import random

import plan_model as P
import reflow_oracle as O
import wave_model as W

KIND, OTHER_KIND = 0, 7
# DAG seed -> (nodes, with a liveset).  Picked on the CPU from the model alone;
# tests/test_wave_model.py asserts what they cover together and one by one.
SEEDS = [(1, 80, False), (2, 200, False), (2, 200, True), (3, 300, True), (6, 120, False), (40, 150, True)]


def fake_key(tag, i):
    return hashlib.sha256(b"%s %d" % (tag, i)).digest()


class Case:
    """One seeded flow and its fill."""

    def __init__(self, seed, n, with_liveset):
        from flowgen import random_dag
        self.rng = random.Random(1000 * seed + n)
        rng = self.rng
        self.nodes = nodes = random_dag(seed, n=n)[1][:-1]
        for f in nodes:  # flowgen makes most nodes done: leave a third of those to evaluate
            f.done = f.done and rng.random() < 0.65
        listed = {id(d) for f in nodes for d in f.deps}
        self.roots = [i for i, f in enumerate(nodes) if id(f) not in listed]
        self.invalid = sorted(rng.sample(range(len(nodes)), len(nodes) // 20))
        self.logical = [k[-1] for k in W.wave_keys(nodes)]
        self.puts, self.other, self.deleted = [], [], []
        for i, ks in enumerate(self.keys()):
            present = [k for k in ks if k != W.ZERO]
            if not P.flow_flags([nodes[i]])[0] & P.F_CACHEABLE or rng.random() < 0.3:
                continue
            mode = rng.choice(["first", "logical", "both", "neither"])
            if mode == "neither":
                self.other.append((present[-1], fake_key(b"other kind", i)))  # cached under another kind only
                if rng.random() < 0.5:
                    self.deleted.append(present[0])                            # and put, then deleted
                continue
            for k in {"first": present[:1], "logical": present[-1:], "both": present}[mode]:
                self.puts.append((k, P.fileset_id(i)))
        self.live_keys = [k for k, _ in self.puts if rng.random() < 0.8] if with_liveset else None

    def keys(self):
        """The key rows as they are now: [physical or zeros, logical] for
        OpExec / OpExtern, [logical] otherwise."""
        out = []
        for f, lg in zip(self.nodes, self.logical):
            if f.op in (O.OP["OpExec"], O.OP["OpExtern"]):
                out.append([f.physical_digest() or W.ZERO, lg])
            else:
                out.append([lg])
        return out


class FlowCase(Case):
    """A given flow (the reference's behavioural ones) as a case: `cached` nodes
    have a value under their logical digest, as testutil.WriteCache leaves it."""

    def __init__(self, nodes, roots, cached, seed=0):
        self.rng = random.Random(seed)
        self.nodes, self.roots, self.invalid = nodes, list(roots), []
        self.logical = [k[-1] for k in W.wave_keys(nodes)]
        self.puts = [(self.logical[i], P.fileset_id(i)) for i in cached]
        self.other, self.deleted, self.live_keys = [], [], None


class ModelTarget:
    """The calls of a scenario on the model alone."""

    def __init__(self, case):
        self.ref = O.InmemoryAssoc()
        self.live = P.Liveset(case.live_keys) if case.live_keys is not None else None
        self.model = W.Wave(case.nodes, case.invalid)

    def put(self, kind, keys, vals):
        for k, v in zip(keys, vals):
            self.ref.put(kind, None, k, v)

    def begin(self, roots, keys, no_cache_extern=False):
        self.model.begin(roots, self.ref, KIND, keys, live=self.live, no_cache_extern=no_cache_extern)

    def step(self, finished, keys):
        self.model.step(finished, self.ref, KIND, keys, live=self.live)

    def reject(self, nodes):
        self.model.reject(nodes)

    def check(self):
        pass


def play(case, target, accept=None, no_cache_extern=False, foreign=0.4, write=0.7):
    """Plays the scenario of `case` on target (a ModelTarget, or one that also
    drives a device object and compares in check()).  accept(node): the
    caller's post-checks of a hit (default: a seeded quarter fails); foreign /
    write: the share of newly computable physical keys, and of the finished
    nodes' keys, that are Put between steps.  Returns what happened: states
    seen, mixed waves, rejected hits, filtered keys, which values, the nodes
    that ran and the hits that were accepted."""
    rng, nodes, m = case.rng, case.nodes, target.model
    seen = {"states": set(), "mixed_wave": 0, "rejected": 0, "filtered": 0, "which": set(), "steps": 0,
            "late_hits": 0, "ran": [], "accepted": []}
    if accept is None:
        def accept(i):
            return rng.random() >= 0.25
    target.put(KIND, [k for k, _ in case.puts], [v for _, v in case.puts])
    target.put(OTHER_KIND, [k for k, _ in case.other], [v for _, v in case.other])
    target.put(KIND, case.deleted, [fake_key(b"short-lived", 0)] * len(case.deleted))
    target.put(KIND, case.deleted, [bytes(32)] * len(case.deleted))

    def note():
        target.check()
        seen["states"] |= set(int(s) for s in m.states)
        last_states = {int(m.states[i]) for i in m.last}
        seen["mixed_wave"] += W.HIT in last_states and W.READY in last_states
        seen["filtered"] += m.keys_filtered
        seen["which"] |= {m.hits[i][0] for i in m.last if m.states[i] == W.HIT}
        seen["late_hits"] += sum(1 for i in m.last if m.states[i] == W.HIT) if seen["steps"] else 0

    target.begin(case.roots, case.keys(), no_cache_extern)
    note()
    while True:
        hits = [int(i) for i in m.list(W.HIT, W.LAST)[0]]
        bad = [i for i in hits if not accept(i)]
        if bad:
            target.reject(bad + bad[:1])  # (one of them listed twice)
            seen["rejected"] += len(bad)
            target.check()
        open_ = [int(i) for i in list(m.list(W.READY)[0]) + list(m.list(W.HIT)[0])]
        if not open_:
            break
        done = [i for i in open_ if rng.random() < 0.6] or open_[:1]
        before = case.keys()
        for i in done:
            seen["ran" if m.states[i] == W.READY else "accepted"].append(i)
            nodes[i].done = True
            if nodes[i].value is None:
                nodes[i].value = W.files("out%d" % i)
        after = case.keys()
        ks, vs = [], []
        for i in done:  # CacheWrite of what finished
            for k in after[i]:
                if k != W.ZERO and rng.random() < write:
                    ks.append(k)
                    vs.append(P.fileset_id(i))
        for i in range(len(nodes)):  # another evaluator cached these consumers under their physical key
            if before[i][0] == W.ZERO and after[i][0] != W.ZERO and rng.random() < foreign:
                ks.append(after[i][0])
                vs.append(P.fileset_id(i))
        target.put(KIND, ks, vs)
        rng.shuffle(done)
        target.step(done + done[:1], after)  # (one of them listed twice)
        seen["steps"] += 1
        note()
    return seen
