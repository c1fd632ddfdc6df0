"""Times the graph change feed beside the incremental step it follows (the
record in DESIGN.md §5 "Change feed"): bench.py's `incremental` DAG --
Dag1000(S, P), 1 % of the leaf File IDs toggled per step -- with rf_timer_*
(HIP events on the context's stream) around, per step,

    step          set_slots_device + recompute_async, no feed open
    step_feed     the same with a feed open (the mark-time record kernel)
    listed        step + rf_graph_feed_poll_device
    scan          step + the poll with RF_FEED_FORCE_SCAN
    lookup        step + rf_graph_feed_lookup_device (liveset + HBM assoc)
    readback      step + rf_graph_get_slots of every job-output slot: what a
                  caller without the feed has to do to learn which keys moved

warm, the variants taking turns step by step, medians of STEPS steps each.
Prints one JSON line.

    python tools/feed_probe.py [S] [P] [STEPS]
"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflow_amd import capi  # noqa: E402
from reflow_amd.workloads import Dag1000  # noqa: E402


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 22075
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 25
    assert steps >= 20, "medians of at least 20 steps"
    dag = Dag1000(S, P)
    a = dag.arrays()
    ctx = capi.Context(0, host_threads=0)
    slots, old, new = dag.change_set(0.01)
    d_slots, d_old, d_new = ctx.upload(slots), ctx.upload(old), ctx.upload(new)
    outs = np.sort(np.asarray(a["out_slot"], dtype=np.uint32))

    def load():
        g = capi.Graph.from_arrays(ctx, a)
        g.set_slots(dag.file_slots, dag.leaf_ids)
        g.recompute(True)
        return g

    class Stepper:
        def __init__(self, g):
            self.g, self.v = g, 0

        def __call__(self):
            ver = d_new if self.v == 0 else d_old
            self.v ^= 1
            self.g.set_slots_device(d_slots.ptr, ver.ptr, len(slots), ctx.stream)
            self.g.recompute_async(False, ctx.stream)

    # one graph per variant, so each keeps its own feed state
    names = ["step", "step_feed", "listed", "scan", "lookup", "readback"]
    graphs = {n: load() for n in names}
    step = {n: Stepper(graphs[n]) for n in names}
    for n in ("step_feed", "listed", "scan", "lookup"):
        graphs[n].feed_open()
    tracked = graphs["listed"].feed_stats().tracked_slots
    cap = tracked
    d_s, d_k, d_v = ctx.alloc(4 * cap), ctx.alloc(32 * cap), ctx.alloc(32 * cap)
    d_st, d_n2 = ctx.alloc(cap), ctx.alloc(16)

    # the lookup's tiers: the keys either direction of the toggle produces --
    # every second one has a value in the assoc, three quarters are live
    g = graphs["lookup"]
    keys = []
    for _ in range(2):
        step["lookup"]()
        ctx.sync()
        keys.append(g.feed_poll()[1])
    n_changed = len(keys[0])
    assert n_changed == len(keys[1]) > 0
    allk = np.concatenate(keys)
    assoc = capi.Assoc(ctx, capacity=2 * len(allk))
    assert (assoc.put(0, allk[::2], allk[::2] | 1) == 0).all()
    m = int(np.ceil(-len(allk) * np.log(0.01) / np.log(2) ** 2))
    live = capi.Bloom.new(ctx, m, 7)
    live.add(allk[np.arange(len(allk)) % 4 != 3])

    def run(n):
        gg = graphs[n]
        ctx.sync()
        ctx.timer_start()
        step[n]()
        if n == "listed":
            gg.feed_poll_device(cap, d_s.ptr, d_k.ptr, d_n2.ptr, stream=ctx.stream)
        elif n == "scan":
            gg.feed_poll_device(cap, d_s.ptr, d_k.ptr, d_n2.ptr, flags=capi.RF_FEED_FORCE_SCAN, stream=ctx.stream)
        elif n == "lookup":
            gg.feed_lookup_device(live, assoc, 0, cap, d_s.ptr, d_k.ptr, d_st.ptr, d_v.ptr, d_n2.ptr,
                                  stream=ctx.stream)
        elif n == "readback":
            gg.get_slots(outs)
        ms = ctx.timer_stop()
        if n == "step_feed":  # (untimed: keeps the feed in the one-step state, its marks recorded)
            gg.feed_poll_device(cap, d_s.ptr, d_k.ptr, d_n2.ptr, stream=ctx.stream)
            ctx.sync()
        return ms

    found = {}
    ms = {n: [] for n in names}
    for i in range(3 + steps):  # three warm rounds
        for n in names:
            t = run(n)
            if i >= 3:
                ms[n].append(t)
            if n in ("listed", "scan", "lookup"):
                found[n] = d_n2.to_numpy(np.uint64).tolist()
                assert found[n] == [n_changed, n_changed], (n, found[n])
    st = {n: graphs[n].feed_stats() for n in ("listed", "scan", "lookup")}
    assert st["listed"].polls_scan == 0 and st["scan"].polls_listed == 0
    status = d_st.to_numpy(np.uint8)[:n_changed]
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(json.dumps({
        "workload": "Dag1000 S=%d P=%d, 1%% leaf File IDs toggled per step" % (S, P),
        "jobs": int(len(outs)), "slots": int(a["n_slots"]), "changed_inputs": int(len(slots)),
        "changed_keys_per_step": int(n_changed), "tracked_slots": int(tracked),
        "feed_device_bytes": int(st["listed"].device_bytes), "steps": steps,
        "median_ms": {n: round(v, 4) for n, v in med.items()},
        "min_ms": {n: round(min(v), 4) for n, v in ms.items()},
        "max_ms": {n: round(max(v), 4) for n, v in ms.items()},
        "poll_listed_ms": round(med["listed"] - med["step_feed"], 4),
        "poll_scan_ms": round(med["scan"] - med["step_feed"], 4),
        "lookup_ms": round(med["lookup"] - med["step_feed"], 4),
        "readback_ms": round(med["readback"] - med["step"], 4),
        "readback_bytes": int(32 * len(outs)),
        "lookup_status_counts": [int((status == k).sum()) for k in (0, 1, 2)],
    }))


if __name__ == "__main__":
    main()
