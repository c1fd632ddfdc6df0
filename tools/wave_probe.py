"""Times the evaluation waves (rf_eval_wave_*) on bench.py's `incremental` DAG
-- Dag1000(S, P), configs[2]'s shape -- beside what a caller had before them
(the record in DESIGN.md §5 "Evaluation waves").

The node graph, flags, key rows (key_slots into the loaded graph's table) and
roots are tools/plan_probe.py's.  Two caches: `full` holds every cacheable
node's keys (every lookup hits), `empty` holds nothing (every lookup misses,
everything has to run).  Measured, each as the median / min / max of REPS
calls after one warm-up, by device events around the call
(rf_timer_start / rf_timer_stop on the context's stream) and by the host
clock around it -- every call ends in a stream synchronise:

    begin       rf_eval_wave_begin from the roots (descent, wave 0 resolved)
    step_B      after a fresh begin, rf_eval_wave_step for the first B nodes of
                wave 0, B = 10^2, 10^4, 10^6: the decrements and the resolved
                next wave
    evaluation  a complete bottom-up evaluation in waves: begin, then per wave
                the host-form lists of the wave's READY and HIT nodes and a
                step that finishes them all
    handover_begin / handover_step_B
                the top-down continuation: rf_eval_wave_begin_states from a
                plan's device states, and the same steps (no lookups)

Baselines on the same box, same process:

    plan_completion_B   what the library offered for a completion before:
                rf_eval_plan_set_flags(DONE) for the B nodes, then a fresh
                rf_eval_plan_run from the roots (empty cache: the walk covers
                everything)
    host_B      16 host threads doing the pending decrements
                (tools/wave_host_bench), plus rf_graph_get_slots of the newly
                ready nodes' key rows and rf_assoc_lookup over them

Checks: the evaluation ends with every node DONE and visits each node once;
the host baseline finds as many ready nodes as the device step.  Prints one
JSON line.

    python tools/wave_probe.py [S] [P] [REPS]
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from plan_probe import node_graph  # noqa: E402
from reflow_amd import capi  # noqa: E402
from reflow_amd.workloads import Dag1000  # noqa: E402

UNSEEN, TODO, READY, HIT, DONE = range(5)
BATCHES = (100, 10_000, 1_000_000)
HOST_BENCH = os.path.join(ROOT, "tools", "wave_host_bench")


def summary(ms):
    dev = [d for d, _ in ms]
    host = [h for _, h in ms]
    return {"device_ms": {"median": round(statistics.median(dev), 4), "min": round(min(dev), 4), "max": round(max(dev), 4)},
            "host_ms": {"median": round(statistics.median(host), 4), "min": round(min(host), 4), "max": round(max(host), 4)}}


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
    prev = g.get_slots(G["key_slots"])
    caches = {"full": capi.Assoc(ctx, capacity=len(prev)), "empty": capi.Assoc(ctx, capacity=1024)}
    assert (caches["full"].put(0, prev, prev | 1) == 0).all()

    def timed(fn):
        ctx.timer_start()
        t0 = time.perf_counter()
        fn()
        host = 1e3 * (time.perf_counter() - t0)
        return ctx.timer_stop(), host

    w = capi.EvalWave(ctx, G["dep_ptr"], G["deps"], G["flags"], G["key_ptr"], G["key_slots"])
    out = {"workload": "Dag1000 S=%d P=%d" % (S, P), "nodes": int(n), "deps": int(len(G["deps"])),
           "keys": int(len(G["key_slots"])), "roots": int(len(roots)), "reps": reps,
           "device_bytes": int(w.stats().device_bytes)}
    wave0 = None
    for name, assoc in caches.items():
        rec = {}
        ms = [timed(lambda: w.begin(roots, assoc, 0, graph=g)) for _ in range(reps + 1)]
        st = w.stats()
        rec["begin"] = dict(summary(ms[1:]), rounds=int(st.rounds), depth=int(st.depth), wave0=int(st.last_wave),
                            looked_up=int(st.looked_up), keys_probed=int(st.keys_probed), counts=list(st.counts))
        if wave0 is None:
            wave0 = np.sort(np.concatenate([w.list(READY, capi.RF_WAVE_LAST)[0], w.list(HIT, capi.RF_WAVE_LAST)[0]]))
        for b in BATCHES:
            fin = wave0[:b]
            ms = []
            for _ in range(reps + 1):
                w.begin(roots, assoc, 0, graph=g)
                ms.append(timed(lambda: w.step(fin, assoc, 0, graph=g)))
            st = w.stats()
            rec["step_%d" % b] = dict(summary(ms[1:]), finished=int(len(fin)), next_wave=int(st.last_wave),
                                      looked_up=int(st.looked_up), keys_probed=int(st.keys_probed))
        # a complete evaluation, wave by wave
        ms, steps_ms, sizes = [], [], []
        for _ in range(min(reps, 3) + 1):
            sizes, per_step = [], []

            def evaluation():
                w.begin(roots, assoc, 0, graph=g)
                while True:
                    s = w.stats()
                    sizes.append(int(s.last_wave))
                    if not s.last_wave:
                        return
                    last = np.concatenate([w.list(READY, capi.RF_WAVE_LAST)[0],
                                           w.list(HIT, capi.RF_WAVE_LAST)[0]])
                    t0 = time.perf_counter()
                    w.step(last, assoc, 0, graph=g)
                    per_step.append(1e3 * (time.perf_counter() - t0))
            ms.append(timed(evaluation))
            steps_ms.append(sum(per_step))
        st = w.stats()
        assert st.counts[DONE] == n and sum(sizes) == n, (list(st.counts), sum(sizes))  # each node in one wave
        rec["evaluation"] = dict(summary(ms[1:]), waves=len(sizes) - 1, largest_wave=max(sizes),
                                 steps_only_host_ms=round(statistics.median(steps_ms[1:]), 4))
        out[name] = rec

    # ---- the parent's completion: set_flags(DONE) + a fresh plan from the roots (empty cache)
    empty = caches["empty"]
    plan = capi.EvalPlan(ctx, G["dep_ptr"], G["deps"], G["flags"], G["key_ptr"], G["key_slots"])
    ms = [timed(lambda: plan.run(roots, empty, 0, graph=g)) for _ in range(reps + 1)]
    st = plan.stats()
    base = {"plan_run": dict(summary(ms[1:]), looked_up=int(st.looked_up), rounds=int(st.rounds), counts=list(st.counts))}
    for b in BATCHES:
        fin = wave0[:b]
        done = G["flags"][fin] | capi.RF_PLAN_F_DONE
        ms = []
        for _ in range(reps + 1):
            plan.set_flags(fin, G["flags"][fin])

            def completion():
                plan.set_flags(fin, done)
                plan.run(roots, empty, 0, graph=g)
            ms.append(timed(completion))
        st = plan.stats()
        base["plan_completion_%d" % b] = dict(summary(ms[1:]), looked_up=int(st.looked_up), ready=int(st.counts[READY]))
        plan.set_flags(fin, G["flags"][fin])
    # ---- the top-down continuation from that plan
    plan.run(roots, empty, 0, graph=g)
    ms = [timed(lambda: w.begin_states(d_states=plan.states_device())) for _ in range(reps + 1)]
    st = w.stats()
    assert w.list(READY, capi.RF_WAVE_LAST)[0].tobytes() == plan.list(READY)[0].tobytes()
    hand = {"handover_begin": dict(summary(ms[1:]), wave0=int(st.last_wave))}
    ready0 = plan.list(READY)[0]
    for b in BATCHES:
        fin = ready0[:b]
        ms = []
        for _ in range(reps + 1):
            w.begin_states(d_states=plan.states_device())
            ms.append(timed(lambda: w.step(fin)))
        st = w.stats()
        assert st.looked_up == 0
        hand["handover_step_%d" % b] = dict(summary(ms[1:]), finished=int(len(fin)), next_wave=int(st.last_wave))
    out["top_down"] = dict(base, **hand)

    # ---- the host: 16 threads for the decrements, get_slots + rf_assoc_lookup for the lookups
    host = {}
    if os.path.exists(HOST_BENCH):
        cons_ptr, cons = capi.eval_wave_consumers(G["dep_ptr"], G["deps"])
        pending0 = np.diff(G["dep_ptr"].astype(np.int64)).astype(np.uint32)
        nkeys = np.diff(G["key_ptr"].astype(np.int64))
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "wave.bin")
            with open(path, "wb") as f:
                fin = wave0[:max(BATCHES)].astype(np.uint32)
                f.write(np.array([n, len(cons), len(fin)], np.uint64).tobytes())
                for a in (cons_ptr, cons, pending0, fin):
                    f.write(np.ascontiguousarray(a).tobytes())
            for b in BATCHES:
                r = subprocess.run([HOST_BENCH, path, "16", str(reps), str(b)], capture_output=True, text=True, check=True)
                rec = json.loads(r.stdout)
                # the lookups of the nodes that step made ready, as the library offered them before
                w.begin(roots, caches["full"], 0, graph=g)
                w.step(wave0[:b], caches["full"], 0, graph=g)
                assert w.stats().last_wave == rec["ready"], (w.stats().last_wave, rec)
                nxt = np.sort(np.concatenate([w.list(READY, capi.RF_WAVE_LAST)[0], w.list(HIT, capi.RF_WAVE_LAST)[0]]))
                nxt = nxt[nkeys[nxt] > 0]
                kp = np.zeros(len(nxt) + 1, np.uint64)
                kp[1:] = np.cumsum(nkeys[nxt])
                first = np.repeat(G["key_ptr"][nxt].astype(np.int64), nkeys[nxt])
                rows = first + np.arange(len(first)) - np.repeat(kp[:-1].astype(np.int64), nkeys[nxt])
                ms = []
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    if len(rows):
                        keys = g.get_slots(G["key_slots"][rows])
                        caches["full"].lookup(0, keys, kp)
                    ms.append(1e3 * (time.perf_counter() - t0))
                rec["lookup_nodes"] = int(len(nxt))
                rec["get_slots_and_assoc_lookup_ms"] = {"median": round(statistics.median(ms[1:]), 4),
                                                        "min": round(min(ms[1:]), 4), "max": round(max(ms[1:]), 4)}
                host["host_%d" % b] = rec
    out["host"] = host
    print(json.dumps(out))


if __name__ == "__main__":
    main()
