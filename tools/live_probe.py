"""Times the GC liveset (rf_liveset_*) on bench.py's `incremental` DAG shape
-- Dag1000(S, P), configs[2]'s graph as tools/plan_probe.py builds it -- beside
the path a caller of the library had before it (the record in DESIGN.md §5
"GC liveset").

Nodes are the DAG's logical jobs, the edges their Deps, the roots the
per-sample externs.  Every node of one kind (default E2, the middle of each
pair's pipeline) is done and holds a Fileset value: a cut of the graph, so the
walk goes from the roots down to it and nothing beneath it is reached.  The
values are sized so that the run's rows (nlive_est) come to about each TARGET
(default 10^6 and 10^7); one row in ten repeats an earlier row of its value.

Per target, wall-clock medians of REPS calls (each ends in a device
synchronise), alternating:

    run            rf_liveset_run
    run_collect    rf_liveset_run + rf_bloom_collect_device over OBJECTS
                   repository objects (the live files and as many others) in
                   the same stream, to its synchronise
    host           what a caller had: a numpy walk of the same graph kind by
                   kind, the Files() dedup on the host (np.unique over one
                   64-bit key per row -- ordinal, first ID word and size mixed
                   -- which is cheaper than comparing whole rows: in the
                   baseline's favour), rf_bloom_new + rf_bloom_add of the
                   distinct IDs, and a compare of the words with the previous
                   filter's on the host
    host_collect   the same + rf_bloom_collect_device

The host path is also the check: states, nlive_est, nlive, livebytes, (m, k)
and every filter word must agree.  Prints one JSON line.

    python tools/live_probe.py [S] [P] [REPS] [KIND] [TARGET ...]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plan_probe import node_graph  # noqa: E402
from reflow_amd import capi  # noqa: E402
from reflow_amd.workloads import Dag1000  # noqa: E402

UNSEEN, WALKED, VALUE = range(3)


def host_walk(G, roots, has):
    """States by a traversal on the host: kinds from the roots down (a kind's Deps are earlier kinds)."""
    n = G["n"]
    reached = np.zeros(n, dtype=bool)
    reached[roots] = True
    state = np.zeros(n, dtype=np.uint8)
    for name in reversed(G["order"]):
        start, count, dl = G["layout"][name]
        r = reached[start:start + count]
        v = r & has[start:start + count]
        walked = r & ~v
        state[start:start + count] = np.where(v, VALUE, np.where(walked, WALKED, UNSEEN))
        for d in dl:
            reached[d[walked]] = True
    return state


def median_ms(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 22075
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    kind = sys.argv[4] if len(sys.argv) > 4 else "E2"
    targets = [int(float(x)) for x in sys.argv[5:]] or [10 ** 6, 10 ** 7]
    dag = Dag1000(S, P)
    G = node_graph(dag)
    n = G["n"]
    ctx = capi.Context(0, host_threads=0)
    xs0, xs_n, _ = G["layout"]["XS"]
    roots = np.arange(xs0, xs0 + xs_n, dtype=np.uint32)
    c0, c_n, _ = G["layout"][kind]
    cut = np.arange(c0, c0 + c_n, dtype=np.uint32)
    has = np.zeros(n, dtype=bool)
    has[cut] = True
    out = {"workload": "Dag1000 S=%d P=%d" % (S, P), "nodes": int(n), "edges": int(len(G["deps"])),
           "roots": int(len(roots)), "cut_kind": kind, "values": int(c_n), "reps": reps, "targets": {}}

    t0 = time.perf_counter()
    L = capi.GcLiveset(ctx, G["dep_ptr"], G["deps"])
    out["open_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    rng = np.random.default_rng(7)
    for target in targets:
        # the values: counts that sum to about target; one row in ten repeats an earlier one of its value
        avg = target / c_n
        edges = np.floor(np.arange(c_n + 1) * avg).astype(np.int64)
        counts = np.diff(edges).astype(np.uint32)
        rows = int(edges[-1])
        ids = rng.integers(0, 1 << 63, size=(rows, 4), dtype=np.int64).view(np.uint64)
        sizes = rng.integers(0, 1 << 30, size=rows).astype(np.int64)
        ordinal = np.repeat(np.arange(c_n, dtype=np.int64), counts)
        first = edges[:-1][ordinal]
        rep = np.flatnonzero((np.arange(rows) % 10 == 9) & (np.arange(rows) > first))
        ids[rep] = ids[first[rep]]
        sizes[rep] = sizes[first[rep]]
        t0 = time.perf_counter()
        L.set_values(cut, counts, ids.view(np.uint8), sizes)
        set_ms = 1e3 * (time.perf_counter() - t0)
        # the repository: the live files and as many others
        n_obj = 2 * rows
        objs = np.concatenate([ids, rng.integers(0, 1 << 63, size=(rows, 4), dtype=np.int64).view(np.uint64)])
        d_objs, d_idx, d_n = ctx.upload(objs.view(np.uint8)), ctx.alloc(8 * n_obj), ctx.alloc(16)

        prev_words = [None]

        def host_path(collect):
            t = [time.perf_counter()]
            state = host_walk(G, roots, has)
            t.append(time.perf_counter())
            contrib = np.flatnonzero(state == VALUE)  # ascending; here: the whole cut, so rows are in arena order
            est = int(counts.sum())
            key = ids[:, 0] ^ (sizes.view(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ \
                (ordinal.view(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
            _, firsts = np.unique(key, return_index=True)
            nlive, livebytes = len(firsts), int(sizes[firsts].sum())
            t.append(time.perf_counter())
            m, k = capi.bloom_estimate(est, 0.001) if est else (64, 1)
            b = capi.Bloom.new(ctx, m, k)
            b.add(ids[firsts].view(np.uint8))
            words = b.words()
            changed = prev_words[0] is None or len(prev_words[0]) != len(words) or not np.array_equal(prev_words[0], words)
            prev_words[0] = words
            t.append(time.perf_counter())
            if collect:
                b.collect_device(d_objs.ptr, None, n_obj, d_idx.ptr, d_n.ptr)
                ctx.sync()
            t.append(time.perf_counter())
            res = dict(state=state, contributions=len(contrib), est=est, nlive=nlive, livebytes=livebytes, m=m, k=k,
                       words=words, changed=changed, dead=int(d_n.to_numpy(np.uint64)[0]) if collect else None)
            b.close()
            return res, [1e3 * (b_ - a_) for a_, b_ in zip(t, t[1:])]

        def device_path(collect):
            t0 = time.perf_counter()
            st = L.run(roots)
            if collect:
                L.filter().collect_device(d_objs.ptr, None, n_obj, d_idx.ptr, d_n.ptr)
                ctx.sync()
            return st, 1e3 * (time.perf_counter() - t0)

        ms = {"run": [], "run_collect": [], "host": [], "host_collect": []}
        parts = []
        want = None
        for rep_i in range(reps + 1):  # the first round is warm-up
            st, a = device_path(False)
            st2, b_ = device_path(True)
            dead_dev = int(d_n.to_numpy(np.uint64)[0])
            want, hp = host_path(False)
            want2, hp2 = host_path(True)
            assert dead_dev == want2["dead"], (dead_dev, want2["dead"])
            if rep_i:
                ms["run"].append(a)
                ms["run_collect"].append(b_)
                ms["host"].append(sum(hp))
                ms["host_collect"].append(sum(hp2))
                parts.append(hp)
        # the check
        assert (L.states() == want["state"]).all()
        assert (st.contributions, st.nlive_est, st.nlive, st.livebytes, st.m, st.k) == \
            (want["contributions"], want["est"], want["nlive"], want["livebytes"], want["m"], want["k"])
        assert (L.filter().words() == want["words"]).all() and st.changed == 0 and not want["changed"]
        rec = {"rows": rows, "nlive": int(st.nlive), "m": int(st.m), "k": int(st.k), "rounds": int(st.rounds),
               "counts": [int(c) for c in st.counts], "objects": n_obj, "dead": dead_dev,
               "set_values_ms": round(set_ms, 3), "device_bytes": int(st.device_bytes),
               "host_parts_ms": {name: round(statistics.median(p[i] for p in parts), 3)
                                 for i, name in enumerate(["walk", "dedup", "bloom_new_add_compare"])}}
        rec.update({k_: median_ms(v) for k_, v in ms.items()})
        out["targets"][str(target)] = rec
        for d in (d_objs, d_idx, d_n):
            d.free()
    L.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
