"""Times the physical keys on the device (rf_physkeys_*) on bench.py's
`incremental` DAG -- Dag1000(S, P), configs[2]'s node graph as
tools/plan_probe.py builds it -- beside the path a caller had before them (the
record in DESIGN.md §5 "Physical keys").

A node's key row is the first of its key_ptr rows where it has two (the kinds
that have a physical key); its suffix is 8 bytes.  The finished nodes are B
deps of the first nodes that have a key row (as many of those as it takes), so
that keys become computable; their values are unmarshalled from JSON on the
device (rf_fileset_unmarshal, not timed: a round needs it either way).

Cases: B = 10^4 and 10^6 with one-file values (material 35 B), B = 10^3 with
10^3-file values.  Measured, each the median / min / max of REPS calls after
one warm-up, host clock around calls that end in a stream synchronise:

    device      rf_physkeys_set_values_forest, then rf_physkeys_update(CONSUMERS),
                and the update's per-pass split by device events
                (rf_physkeys_stats.last_ms)
    before      rf_fileset_forest_copy, the materials built on 16 host threads
                (tools/physkeys_host_bench), rf_sha256_arena over them, the
                upload of the digests

Check: the rows the device wrote equal the digests of the host path, consumer
by consumer.  Prints one JSON line.

    python tools/physkeys_probe.py [S] [P] [REPS]
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

HOST_BENCH = os.path.join(ROOT, "tools", "physkeys_host_bench")
CASES = [("one_file_1e4", 10_000, 1), ("one_file_1e6", 1_000_000, 1), ("thousand_files_1e3", 1_000, 1_000)]
PASSES = ("affected", "measure_readback", "segments", "gather", "k1", "scatter")


def stat(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def documents(b, files):
    """b canonical documents of `files` entries each; every ID differs."""
    docs = []
    for d in range(b):
        ents = []
        for k in range(files):
            fid = (d * files + k + 1).to_bytes(8, "little") * 4
            ents.append(b'"f%06d":{"ID":"sha256:%s","Size":1}' % (k, fid.hex().encode()) if files > 1 else
                        b'"f":{"ID":"sha256:%s","Size":1}' % fid.hex().encode())
        docs.append(b'{"Fileset":{' + b",".join(ents) + b'}}')
    return docs


def finished_nodes(G, rowed, b):
    """The first b distinct deps of the first m nodes that have a row, m as small as doubling finds it."""
    dep_ptr, deps = G["dep_ptr"].astype(np.int64), G["deps"]
    m = max(b // 4, 1)
    while True:
        c = rowed[:m]
        lens = dep_ptr[c + 1] - dep_ptr[c]
        before = np.cumsum(lens) - lens
        idx = np.repeat(dep_ptr[c] - before, lens) + np.arange(int(lens.sum()))
        fin = np.unique(deps[idx])
        if len(fin) >= b or m >= len(rowed):
            return fin[:b].astype(np.uint32)
        m *= 2


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 22075
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    G = node_graph(Dag1000(S, P))
    n = G["n"]
    nkeys = np.diff(G["key_ptr"].astype(np.int64))
    phys_row = np.where(nkeys == 2, G["key_ptr"][:-1], np.uint64(capi.RF_PHYS_NO_ROW)).astype(np.uint64)
    n_rows = int(G["key_ptr"][-1])
    suffix_ptr = np.arange(n + 1, dtype=np.uint64) * 8
    suffix = np.arange(n, dtype=np.uint64).view(np.uint8)
    cons_ptr, cons = capi.eval_wave_consumers(G["dep_ptr"], G["deps"])
    rowed = np.nonzero(nkeys == 2)[0]
    ctx = capi.Context(0, host_threads=16)
    pk = capi.PhysKeys(ctx, G["dep_ptr"], G["deps"], phys_row, suffix_ptr=suffix_ptr, suffix=suffix)
    d_keys = ctx.alloc(32 * n_rows)
    d_keys.zero()
    out = {"workload": "Dag1000 S=%d P=%d" % (S, P), "nodes": int(n), "deps": int(len(G["deps"])),
           "key_rows": n_rows, "nodes_with_row": int((nkeys == 2).sum()), "reps": reps, "cases": {}}
    for name, b, files in CASES:
        fin = finished_nodes(G, rowed, b)
        docs = documents(len(fin), files)
        t0 = time.perf_counter()
        forest = capi.FilesetForest.from_host(ctx, docs)
        rec = {"finished": int(len(fin)), "files_per_value": files, "json_bytes": sum(len(d) for d in docs),
               "unmarshal_ms_untimed_part": round(1e3 * (time.perf_counter() - t0), 3)}
        assert forest.n_accepted == len(fin)
        set_ms, upd_ms, split = [], [], {p: [] for p in PASSES}
        o = None
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            pk.set_values_forest(fin, forest)
            t1 = time.perf_counter()
            o = pk.update(fin, capi.RF_PHYS_CONSUMERS, d_keys.ptr, n_rows)
            t2 = time.perf_counter()
            set_ms.append(1e3 * (t1 - t0))
            upd_ms.append(1e3 * (t2 - t1))
            st = pk.stats()
            for i, p in enumerate(PASSES):
                split[p].append(st.last_ms[i])
        rec["device"] = {"set_values_forest_ms": stat(set_ms[1:]), "update_ms": stat(upd_ms[1:]),
                         "total_ms": stat([a + c for a, c in zip(set_ms[1:], upd_ms[1:])]),
                         "update_passes_ms": {p: stat(v[1:]) for p, v in split.items()},
                         "affected": int(o.affected), "keys_written": int(o.keys_written),
                         "keys_zeroed": int(o.keys_zeroed), "material_bytes": int(o.material_bytes)}
        st = pk.stats()
        rec["store"] = {"arena_bytes": int(st.arena_bytes), "stale_bytes": int(st.stale_bytes),
                        "device_bytes": int(st.device_bytes)}
        # ---- the path before: copy, host materials, rf_sha256_arena, upload
        copy_ms = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            s = forest.copy()
            copy_ms.append(1e3 * (time.perf_counter() - t0))
        before = {"forest_copy_ms": stat(copy_ms[1:])}
        if os.path.exists(HOST_BENCH):
            with tempfile.TemporaryDirectory() as tmp:
                src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
                with open(src, "wb") as f:
                    f.write(np.array([n, len(cons), len(fin), forest.n_nodes, forest.n_entries, forest.path_bytes,
                                      len(suffix)], np.uint64).tobytes())
                    for a in (G["dep_ptr"], G["deps"], cons_ptr, cons, phys_row, suffix_ptr, suffix, fin,
                              s["doc_node_ptr"], s["node_depth"], s["entry_ptr"], s["path_off"], s["paths"], s["ids32"]):
                        f.write(np.ascontiguousarray(a).tobytes())
                r = subprocess.run([HOST_BENCH, src, dst, "16", str(reps)], capture_output=True, text=True, check=True)
                before["host_materials"] = json.loads(r.stdout)
                raw = np.fromfile(dst, dtype=np.uint8)
            k, a = (int(x) for x in raw[:16].view(np.uint64))
            rows, offs, lens = (raw[16 + 8 * k * i:16 + 8 * k * (i + 1)].view(np.uint64) for i in range(3))
            arena = raw[16 + 24 * k:16 + 24 * k + a]
            sha_ms, up_ms, dig = [], [], None
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                dig = ctx.sha256_arena(arena, offs, lens)
                t1 = time.perf_counter()
                buf = ctx.upload(dig)
                t2 = time.perf_counter()
                buf.free()
                sha_ms.append(1e3 * (t1 - t0))
                up_ms.append(1e3 * (t2 - t1))
            before["sha256_arena_ms"] = stat(sha_ms[1:])
            before["upload_rows_ms"] = stat(up_ms[1:])
            before["total_ms"] = round(before["forest_copy_ms"]["median"] + before["host_materials"]["median_ms"] +
                                       before["sha256_arena_ms"]["median"] + before["upload_rows_ms"]["median"], 4)
            got = d_keys.to_numpy(np.uint8, 32 * n_rows).reshape(-1, 32)
            assert k == o.keys_written and (got[rows.astype(np.int64)] == dig).all(), "device rows differ from the host path"
            rec["rows_equal_host_path"] = True
        rec["before"] = before
        out["cases"][name] = rec
        forest.close()
        pk.clear_values(fin)
        d_keys.zero()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
