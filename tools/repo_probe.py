"""Times the repository index (rf_repo_*) on bench.py's `incremental` DAG shape
-- Dag1000(S, P), configs[2]'s graph as tools/plan_probe.py builds it -- beside
the same answers computed on the host (the record in DESIGN.md §5 "Repository
index").

The plan is plan_probe's `changed_logical_keys_only` state: the cache holds the
logical keys, configs[2]'s 1 % change step has run, so the walk goes down to the
changed pairs and leaves hits, TODO and READY nodes.  Every hit holds a Fileset
value (what the caller unmarshalled from the cache), with the liveset probe's
distribution: the rows come to about each TARGET (default 10^6), one row in ten
repeats an earlier row of its value.  The repository holds every second
distinct file.

Per target, wall-clock medians of REPS calls (each ends in a device
synchronise):

    missing        rf_repo_missing_device over the hits' values (rows, counts
                   and outputs in device memory)
    need_transfer  rf_eval_plan_list_device of the READY nodes, then
                   rf_repo_need_transfer_device over that list, device to device
    host_missing / host_need_transfer
                   the same answers with numpy on one thread: the Files() dedup
                   as np.unique over one 64-bit key per row (group, first ID
                   word and size mixed -- cheaper than comparing whole rows: in
                   the baseline's favour), existence by a binary search of the
                   first ID word among the repository's, per-group sums by
                   bincount.  (tools/repo_host_bench.cpp times the C++
                   mirror's FlatMap on 16 threads over the same distribution.)

The host path is also the check: n_files, n_missing, missing_bytes per group
and the totals must agree.  It is an approximate check: it tells files apart by
a mixed 64-bit key and tests existence by the first ID word, so a collision
among the random IDs (about 10^-5 likely at 10^7 rows) would show as a false
failure; tools/repo_host_bench.cpp and the tests compare whole keys.  Prints one JSON line.

    python tools/repo_probe.py [S] [P] [REPS] [TARGET ...]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plan_probe import HIT, READY, node_graph  # noqa: E402
from reflow_amd import capi  # noqa: E402
from reflow_amd.workloads import Dag1000  # noqa: E402


def median_ms(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def host_missing(group, ids, sizes, n_groups, repo_words):
    """(n_files, n_missing, missing_bytes) per group, on the host."""
    key = ids[:, 0] ^ (sizes.view(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ \
        (group.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
    _, firsts = np.unique(key, return_index=True)
    w = ids[firsts, 0]
    at = np.searchsorted(repo_words, w)
    present = (at < len(repo_words)) & (repo_words[np.minimum(at, len(repo_words) - 1)] == w)
    g = group[firsts]
    n_files = np.bincount(g, minlength=n_groups).astype(np.uint32)
    n_missing = np.bincount(g[~present], minlength=n_groups).astype(np.uint32)
    mbytes = np.bincount(g[~present], weights=sizes[firsts][~present].astype(np.float64),
                         minlength=n_groups).astype(np.int64)
    return n_files, n_missing, mbytes


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 22075
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    targets = [int(float(x)) for x in sys.argv[4:]] or [10 ** 6]
    dag = Dag1000(S, P)
    G = node_graph(dag)
    n = G["n"]
    ctx = capi.Context(0, host_threads=0)
    g = capi.Graph.from_arrays(ctx, dag.arrays())
    g.set_slots(dag.file_slots, dag.leaf_ids)
    g.recompute(True)
    xs0, xs_n, _ = G["layout"]["XS"]
    roots = np.arange(xs0, xs0 + xs_n, dtype=np.uint32)
    # the previous run's cache, logical keys only; then the change step
    kp = G["key_ptr"].astype(np.int64)
    logical = (kp[1:][np.diff(kp) > 0] - 1)
    prev = g.get_slots(G["key_slots"][logical])
    assoc = capi.Assoc(ctx, capacity=len(prev))
    assert (assoc.put(0, prev, prev | 1) == 0).all()
    slots, _, new = dag.change_set(0.01)
    g.set_slots(slots, new)
    g.recompute(False)
    plan = capi.EvalPlan(ctx, G["dep_ptr"], G["deps"], G["flags"], G["key_ptr"], G["key_slots"])
    plan.run(roots, assoc, 0, graph=g)
    state = plan.states()
    hits = np.flatnonzero(state == HIT).astype(np.uint32)
    ready = np.flatnonzero(state == READY).astype(np.uint32)
    out = {"workload": "Dag1000 S=%d P=%d" % (S, P), "nodes": int(n), "edges": int(len(G["deps"])),
           "hits": int(len(hits)), "ready": int(len(ready)), "reps": reps, "targets": {}}
    dep_ptr = G["dep_ptr"].astype(np.int64)
    L = capi.GcLiveset(ctx, G["dep_ptr"], G["deps"])
    rng = np.random.default_rng(7)
    H = len(hits)
    for target in targets:
        avg = target / max(H, 1)
        edges = np.floor(np.arange(H + 1) * avg).astype(np.int64)
        counts = np.diff(edges).astype(np.uint32)
        rows = int(edges[-1])
        ids = rng.integers(0, 1 << 63, size=(rows, 4), dtype=np.int64).view(np.uint64)
        sizes = rng.integers(0, 1 << 30, size=rows).astype(np.int64)
        ordinal = np.repeat(np.arange(H, dtype=np.int64), counts)
        first = edges[:-1][ordinal]
        rep = np.flatnonzero((np.arange(rows) % 10 == 9) & (np.arange(rows) > first))
        ids[rep] = ids[first[rep]]
        sizes[rep] = sizes[first[rep]]
        L.set_values(hits, counts, ids.view(np.uint8), sizes)
        # the repository: every second distinct file
        _, uniq = np.unique(ids[:, 0], return_index=True)
        held = np.sort(uniq)[::2]
        repo = capi.Repo(ctx, capacity=len(held))
        t0 = time.perf_counter()
        assert (repo.put(ids[held].view(np.uint8), sizes[held]) == 0).all()
        put_ms = 1e3 * (time.perf_counter() - t0)
        repo_words = np.sort(ids[held, 0])
        d_counts, d_ids, d_sizes = ctx.upload(counts), ctx.upload(ids.view(np.uint8)), ctx.upload(sizes)
        # need_transfer's rows on the host: the arena rows of the ready nodes' deps, in edge order
        r_deg = (dep_ptr[ready + 1] - dep_ptr[ready]).astype(np.int64)
        e_idx = np.repeat(dep_ptr[ready], r_deg) + (np.arange(int(r_deg.sum())) - np.repeat(np.cumsum(r_deg) - r_deg, r_deg))
        e_dep = G["deps"][e_idx].astype(np.int64)
        e_grp = np.repeat(np.arange(len(ready), dtype=np.int64), r_deg)
        pos = np.full(n, -1, dtype=np.int64)
        pos[hits] = np.arange(H)
        assert (pos[e_dep] >= 0).all()  # a ready node's deps are hits: they have values
        e_cnt = counts[pos[e_dep]].astype(np.int64)
        nt_rows = int(e_cnt.sum())
        nt_src = np.repeat(edges[:-1][pos[e_dep]], e_cnt) + (np.arange(nt_rows) - np.repeat(np.cumsum(e_cnt) - e_cnt, e_cnt))
        nt_grp = np.repeat(e_grp, e_cnt)

        def outs(groups, cap):
            o = capi.RepoMissingOut()
            bufs = dict(n_files=ctx.alloc(4 * max(groups, 1)), n_missing=ctx.alloc(4 * max(groups, 1)),
                        missing_bytes=ctx.alloc(8 * max(groups, 1)), status=ctx.alloc(4 * max(groups, 1)),
                        miss_ptr=ctx.alloc(8 * (groups + 1)), miss_ids32=ctx.alloc(32 * max(cap, 1)),
                        miss_sizes=ctx.alloc(8 * max(cap, 1)), n_listed=ctx.alloc(8))
            for k_, b in bufs.items():
                setattr(o, k_, b.ptr)
            o.cap = cap
            return o, bufs

        o_m, b_m = outs(H, rows)
        o_t, b_t = outs(len(ready), nt_rows)
        d_ready, d_found = ctx.alloc(4 * max(len(ready), 1)), ctx.alloc(8)
        ms = {"missing": [], "need_transfer": [], "host_missing": [], "host_need_transfer": []}
        for rep_i in range(reps + 1):  # the first round is warm-up
            t0 = time.perf_counter()
            repo.missing_device(d_counts.ptr, H, d_ids.ptr, d_sizes.ptr, rows, o_m)
            ctx.sync()
            t1 = time.perf_counter()
            plan.list_device(READY, len(ready), d_ready.ptr, None, None, None, d_found.ptr)
            repo.need_transfer_device(L, d_ready.ptr, len(ready), o_t)
            ctx.sync()
            t2 = time.perf_counter()
            want_m = host_missing(ordinal, ids, sizes, H, repo_words)
            t3 = time.perf_counter()
            want_t = host_missing(nt_grp, ids[nt_src], sizes[nt_src], len(ready), repo_words)
            t4 = time.perf_counter()
            if rep_i:
                for k_, v in zip(ms, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    ms[k_].append(1e3 * v)
        # the check
        for bufs, want, groups in ((b_m, want_m, H), (b_t, want_t, len(ready))):
            assert (bufs["n_files"].to_numpy(np.uint32)[:groups] == want[0]).all()
            assert (bufs["n_missing"].to_numpy(np.uint32)[:groups] == want[1]).all()
            assert (bufs["missing_bytes"].to_numpy(np.int64)[:groups] == want[2]).all()
            assert int(bufs["n_listed"].to_numpy(np.uint64)[0]) == int(want[1].sum())
        assert (b_t["status"].to_numpy(np.int32)[:len(ready)] == 0).all()
        st = repo.stats()
        rec = {"rows": rows, "files": int(want_m[0].sum()), "missing_files": int(want_m[1].sum()),
               "need_transfer_rows": nt_rows, "need_transfer_missing": int(want_t[1].sum()),
               "objects": int(st.objects), "capacity": int(st.capacity), "put_ms": round(put_ms, 3),
               "device_bytes": int(st.device_bytes)}
        rec.update({k_: median_ms(v) for k_, v in ms.items()})
        out["targets"][str(target)] = rec
        for b in list(b_m.values()) + list(b_t.values()) + [d_counts, d_ids, d_sizes, d_ready, d_found]:
            b.free()
        repo.close()
    L.close()
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
