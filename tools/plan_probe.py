"""Times the evaluation plan (rf_eval_plan_*) on bench.py's `incremental` DAG
-- Dag1000(S, P), configs[2]'s shape -- beside the path a caller had before it
(the record in DESIGN.md §5 "Evaluation plan").

Nodes are the DAG's logical jobs; a node's Deps are the producers of its
job's holes; its cache keys are its physical slot (execs and externs) and its
logical slot in the loaded graph's table (key_slots); the assoc holds every
cacheable node's keys as the previous run left them; the roots are the
per-sample externs.  Three states:

    cached     everything is cached: the roots hit
    nce        the same under NoCacheExtern: the externs run, the merges hit
    changed    after the 1 % change step of configs[2] (the externs' physical
               keys do not depend on the leaf File IDs: the roots still hit)
    changed_logical_keys_only
               the same against a cache that holds the logical keys only:
               the moved keys miss and the walk goes down to the changed pairs

For each, wall-clock medians of REPS runs of rf_eval_plan_run (keys from the
graph) with round_batch 1, 4, 8 and D (RF_PLAN_BATCH at open), the rounds, the
nodes looked up and keys probed, and the host-form lists of hits and ready
nodes.  The baseline is what the library offered before: rf_graph_get_slots
of every cacheable node's keys, rf_assoc_lookup over them, and a traversal on
the host (numpy, kind by kind from the roots down).  That traversal is also
the check: every run's states must equal it.  Prints one JSON line.

    python tools/plan_probe.py [S] [P] [REPS]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflow_amd import capi  # noqa: E402
from reflow_amd.workloads import Dag1000  # noqa: E402

CACHEABLE = ("R0", "R1", "E1", "E2", "E3", "ES", "XS")
PHYSICAL = {"R1": "pR1", "E1": "pE1", "E2": "pE2", "E3": "pE3", "ES": "pES", "XS": "pXS"}
UNSEEN, TODO, READY, HIT, DONE = range(5)


def node_graph(dag):
    """The logical jobs as nodes (node = logical slot - 2Q), kind by kind in
    creation order: CSR of Deps, flags, key_ptr, key_slots, per-kind layout."""
    base = 2 * dag.Q
    order = [k for k in dag.kinds if not k.startswith("p")]
    n = dag.n_logical_slots
    deg = np.zeros(n, dtype=np.uint64)
    nkeys = np.zeros(n, dtype=np.uint64)
    flags = np.zeros(n, dtype=np.uint8)
    deps, key_slots, layout = [], [], {}
    for name in order:
        kk = dag.kinds[name]
        start = int(kk.out_slot[0]) - base
        assert (kk.out_slot == np.arange(start, start + kk.count) + base).all()
        dl = [sl.astype(np.int64) - base for _, sl in kk.holes if int(sl[0]) >= base]
        layout[name] = (start, kk.count, dl)
        deg[start:start + kk.count] = len(dl)
        if dl:
            deps.append(np.stack(dl, axis=1).reshape(-1))
        if name in CACHEABLE:
            flags[start:start + kk.count] = capi.RF_PLAN_F_CACHEABLE | (capi.RF_PLAN_F_EXTERN if name == "XS" else 0)
            cols = ([dag.kinds[PHYSICAL[name]].out_slot] if name in PHYSICAL else []) + [kk.out_slot]
            nkeys[start:start + kk.count] = len(cols)
            key_slots.append(np.stack(cols, axis=1).reshape(-1))
    dep_ptr = np.zeros(n + 1, dtype=np.uint64)
    dep_ptr[1:] = np.cumsum(deg)
    key_ptr = np.zeros(n + 1, dtype=np.uint64)
    key_ptr[1:] = np.cumsum(nkeys)
    return dict(n=n, order=order, layout=layout, dep_ptr=dep_ptr, deps=np.concatenate(deps).astype(np.uint32),
                flags=flags, key_ptr=key_ptr, key_slots=np.concatenate(key_slots).astype(np.uint32))


def host_plan(G, roots, hit):
    """States by a traversal on the host: kinds from the roots down (a kind's
    Deps are earlier kinds), then READY bottom-up."""
    n = G["n"]
    reached = np.zeros(n, dtype=bool)
    reached[roots] = True
    state = np.zeros(n, dtype=np.uint8)
    for name in reversed(G["order"]):
        start, count, dl = G["layout"][name]
        r = reached[start:start + count]
        h = r & hit[start:start + count]
        miss = r & ~h
        state[start:start + count] = np.where(h, HIT, np.where(miss, TODO, UNSEEN))
        for d in dl:
            reached[d[miss]] = True
    for name in G["order"]:
        start, count, dl = G["layout"][name]
        ok = state[start:start + count] == TODO
        for d in dl:
            ok &= state[d] == HIT
        state[start:start + count][ok] = READY
    return state


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 22075
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    dag = Dag1000(S, P)
    G = node_graph(dag)
    ctx = capi.Context(0, host_threads=0)
    g = capi.Graph.from_arrays(ctx, dag.arrays())
    g.set_slots(dag.file_slots, dag.leaf_ids)
    g.recompute(True)
    n = G["n"]
    xs0, xs_n, _ = G["layout"]["XS"]
    roots = np.arange(xs0, xs0 + xs_n, dtype=np.uint32)
    has_keys = np.flatnonzero(np.diff(G["key_ptr"].astype(np.int64)) > 0)
    kp_c = np.zeros(len(has_keys) + 1, dtype=np.uint64)  # the cacheable nodes' key_ptr, packed
    kp_c[1:] = np.cumsum(np.diff(G["key_ptr"].astype(np.int64))[has_keys])

    # the previous run's cache: every cacheable node's keys, value = key | 1
    prev = g.get_slots(G["key_slots"])
    assoc = capi.Assoc(ctx, capacity=len(prev))
    assert (assoc.put(0, prev, prev | 1) == 0).all()

    def baseline(nce, assoc):
        t0 = time.perf_counter()
        rows = g.get_slots(G["key_slots"])
        which = assoc.lookup(0, rows, kp_c)[0]
        t1 = time.perf_counter()
        hit = np.zeros(n, dtype=bool)
        hit[has_keys] = which >= 0
        if nce:  # no extern, no root; nothing is above an extern here, so nothing else is dirty
            hit[xs0:xs0 + xs_n] = False
        state = host_plan(G, roots, hit)
        t2 = time.perf_counter()
        return state, 1e3 * (t1 - t0), 1e3 * (t2 - t1)

    def measure(label, nce, out, assoc):
        want, ms_lookup, ms_walk = baseline(nce, assoc)
        rec = {"baseline_get_slots_and_assoc_lookup_ms": round(ms_lookup, 3), "baseline_host_walk_ms": round(ms_walk, 3),
               "counts": [int((want == s).sum()) for s in range(5)], "run_ms": {}}
        for batch in (1, 4, 8, 0):
            os.environ["RF_PLAN_BATCH"] = str(batch)
            p = capi.EvalPlan(ctx, G["dep_ptr"], G["deps"], G["flags"], G["key_ptr"], G["key_slots"])
            ms = []
            for _ in range(reps + 1):  # the first run is warm-up (and computes the dirty bits)
                t0 = time.perf_counter()
                p.run(roots, assoc, 0, graph=g, no_cache_extern=nce)
                ms.append(1e3 * (time.perf_counter() - t0))
            st = p.stats()
            assert (p.states() == want).all(), (label, batch)
            assert list(st.counts) == rec["counts"]
            key = "D" if batch == 0 else str(batch)
            rec["run_ms"][key] = {"median": round(statistics.median(ms[1:]), 3), "min": round(min(ms[1:]), 3),
                                  "max": round(max(ms[1:]), 3), "rounds": int(st.rounds)}
            if batch == 4:
                rec.update(depth=int(st.depth), looked_up=int(st.looked_up), keys_probed=int(st.keys_probed),
                           round_lanes=int(st.round_lanes), device_bytes=int(st.device_bytes))
                for name, state in (("list_hits_ms", HIT), ("list_ready_ms", READY)):
                    t0 = time.perf_counter()
                    nodes = p.list(state, cap=rec["counts"][state])[0]
                    rec[name] = round(1e3 * (time.perf_counter() - t0), 3)
                    assert (nodes == np.flatnonzero(want == state)).all()
            p.close()
        out[label] = rec

    out = {"workload": "Dag1000 S=%d P=%d" % (S, P), "nodes": int(n), "deps": int(len(G["deps"])),
           "keys": int(len(G["key_slots"])), "roots": int(len(roots)), "reps": reps}
    # the same cache without the physical keys (they do not depend on the leaf
    # File IDs here, so with them the externs still hit after the change step)
    logical = (kp_c[1:] - 1).astype(np.int64)
    assoc_logical = capi.Assoc(ctx, capacity=len(logical))
    assert (assoc_logical.put(0, prev[logical], prev[logical] | 1) == 0).all()
    measure("cached", False, out, assoc)
    measure("nce", True, out, assoc)
    slots, _, new = dag.change_set(0.01)
    g.set_slots(slots, new)
    g.recompute(False)
    out["changed_inputs"] = int(len(slots))
    measure("changed", False, out, assoc)
    measure("changed_logical_keys_only", False, out, assoc_logical)
    os.environ.pop("RF_PLAN_BATCH", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
