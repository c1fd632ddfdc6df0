"""Times the cache write on the device (DESIGN.md §5 "Cache write"): marshal
plus value digests in the device form (rf_fileset_value_digest_device's steps,
the File IDs already in HBM) beside the host form that existed before it
(rf_fileset_value_digest_batch: the host marshals every value into a string,
uploads the JSON and hashes it), on three shapes:

    a   10^5 values of one file "."           (1000align's exec outputs)
    b   10^3 values of 10^3 files
    c   one value of 10^5 files               (a single SHA-256 chain)

Per shape REPS runs after one warm-up, host clock around each call (every call
ends in a stream synchronise); the device form split into flatten + sort /
upload + length + scan + read-back / arena + emit (rf_json_batch_times) and K1
(rf_json_batch_digests_device).  The digests of both forms must be equal.

With `write`: a complete rf_eval_wave_cache_write over bench.py's
`incremental` DAG -- Dag1000(S, P), configs[2]'s wave shape -- for the first
B = 10^4 and 10^6 finished nodes of wave 0, beside the key gather on the host
(rf_graph_get_slots of the nodes' key rows) plus rf_assoc_put + rf_repo_put.

Writes one JSON record to profiles/cwrite/<name>.json and prints it.

    python tools/cwrite_probe.py NAME [REPS] [write [S] [P]]
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reflow_amd import capi  # noqa: E402

OUT_DIR = os.path.join(ROOT, "profiles", "cwrite")


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


class Flat:
    """n_values Map filesets of `files` entries each, as an rf_fileset_tree built
    with numpy (paths of one width in one blob, keys in order)."""

    def __init__(self, n_values, files, one_dot=False):
        e = n_values * files
        rng = np.random.default_rng(7)
        if one_dot:
            self.blob = np.frombuffer(b".", np.uint8).copy()
            addr = np.full(e, self.blob.ctypes.data, np.uint64)
            lens = np.ones(e, np.uint32)
        else:
            text = "".join("d%03d/f%07d.bam" % (i % 97, i) for i in range(files)).encode()
            width = len(text) // files
            self.blob = np.frombuffer(text, np.uint8).copy()
            addr = np.tile(self.blob.ctypes.data + width * np.arange(files, dtype=np.uint64), n_values)
            lens = np.full(e, width, np.uint32)
            order = np.argsort([text[width * i:width * i + width] for i in range(files)], kind="stable")
            addr = addr.reshape(n_values, files)[:, order].reshape(-1).copy()  # bytewise order: no host sort
        self.keep = dict(lp=np.zeros(n_values + 1, np.uint64), lc=np.zeros(1, np.uint32),
                         ep=np.arange(0, e + 1, files, dtype=np.uint64), pp=addr, pl=lens,
                         ids=rng.integers(1, 256, size=32 * e, dtype=np.uint8), sz=np.arange(e, dtype=np.int64))
        k = self.keep
        self.tree = capi.FilesetTree(n_values, k["lp"].ctypes.data, k["lc"].ctypes.data, k["ep"].ctypes.data,
                                     k["pp"].ctypes.data, k["pl"].ctypes.data, k["ids"].ctypes.data, k["sz"].ctypes.data)
        self.roots = np.arange(n_values, dtype=np.uint32)
        self.n, self.entries = n_values, e


def shape(ctx, name, flat, reps):
    L = capi.lib()
    n = flat.n
    d_ids = ctx.upload(flat.keep["ids"])  # the device form's IDs are in HBM already (K1's out32)
    d_out = ctx.alloc(32 * n)
    no_ids = capi.FilesetTree(flat.tree.n_nodes, flat.tree.list_ptr, flat.tree.list_child, flat.tree.entry_ptr,
                              flat.tree.paths, flat.tree.path_lens, None, flat.tree.sizes)
    dev, parts, host = [], [], []
    host_out = np.zeros(32 * n, np.uint8)
    json_bytes = pieces = 0
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        b = capi.JsonBatch(ctx, tree=no_ids, roots=flat.roots, d_ids32=d_ids.ptr)
        t1 = time.perf_counter()
        b.digests_device(d_out.ptr)
        t2 = time.perf_counter()
        dev.append(1e3 * (t2 - t0))
        parts.append(b.times() + (1e3 * (t2 - t1),))
        json_bytes, pieces = b.total_bytes, b.n_pieces
        b.close()
        t0 = time.perf_counter()
        capi._check(L.rf_fileset_value_digest_batch(ctx.handle, ctypes.byref(flat.tree), flat.roots.ctypes.data, n,
                                                    host_out.ctypes.data))
        host.append(1e3 * (time.perf_counter() - t0))
    assert d_out.to_numpy(np.uint8, 32 * n).tobytes() == host_out.tobytes(), name
    d_ids.free()
    d_out.free()
    cols = list(zip(*parts[1:]))
    return {"values": n, "entries": flat.entries, "json_bytes": int(json_bytes), "pieces": int(pieces),
            "device_form_ms": stat(dev[1:]), "host_form_ms": stat(host[1:]),
            "device_split_ms": {"flatten_sort": stat(cols[0]), "upload_length_scan_readback": stat(cols[1]),
                                "arena_emit": stat(cols[2]), "k1": stat(cols[3])},
            "device_slowest_beats_host_fastest": max(dev[1:]) < min(host[1:])}


def write_probe(ctx, reps, S, P):
    from plan_probe import node_graph
    from reflow_amd.workloads import Dag1000
    READY, HIT = 2, 3
    dag = Dag1000(S, P)
    G = node_graph(dag)
    g = capi.Graph.from_arrays(ctx, dag.arrays())
    g.set_slots(dag.file_slots, dag.leaf_ids)
    g.recompute(True)
    xs0, xs_n, _ = G["layout"]["XS"]
    roots = np.arange(xs0, xs0 + xs_n, dtype=np.uint32)
    w = capi.EvalWave(ctx, G["dep_ptr"], G["deps"], G["flags"], G["key_ptr"], G["key_slots"])
    empty = capi.Assoc(ctx, 1024)
    w.begin(roots, empty, 0, graph=g)
    wave0 = np.sort(np.concatenate([w.list(READY, capi.RF_WAVE_LAST)[0], w.list(HIT, capi.RF_WAVE_LAST)[0]]))
    nkeys = np.diff(G["key_ptr"].astype(np.int64))
    cacheable = (G["flags"] & capi.RF_PLAN_F_CACHEABLE) != 0
    wave0 = wave0[cacheable[wave0] & (nkeys[wave0] > 0)]
    out = {"workload": "Dag1000 S=%d P=%d" % (S, P), "nodes": int(G["n"]), "wave0_cacheable": int(len(wave0))}
    rng = np.random.default_rng(3)
    for B in (10_000, 1_000_000):
        fin = wave0[:B]
        if not len(fin):
            continue
        w.begin(roots, empty, 0, graph=g)
        w.step(fin, empty, 0, graph=g)
        fsids = rng.integers(1, 256, size=32 * len(fin), dtype=np.uint8)
        sizes = rng.integers(2, 1 << 20, size=len(fin), dtype=np.int64)
        d_f, d_s = ctx.upload(fsids), ctx.upload(sizes)
        first = np.repeat(G["key_ptr"][fin].astype(np.int64), nkeys[fin])
        kp = np.concatenate([[0], np.cumsum(nkeys[fin])])
        rows = first + np.arange(len(first)) - np.repeat(kp[:-1], nkeys[fin])
        dev, host, puts = [], [], 0
        for _ in range(reps + 1):
            a, r = capi.Assoc(ctx, 1024), capi.Repo(ctx, 0)
            t0 = time.perf_counter()
            o, _ = w.cache_write(fin, d_f.ptr, d_s.ptr, a, 0, graph=g, repo=r, per_node=False)
            dev.append(1e3 * (time.perf_counter() - t0))
            puts = int(o.keys_put)
            on_device = a.count(0)[0], r.stats().objects
            a.close()
            r.close()
            a, r = capi.Assoc(ctx, 1024), capi.Repo(ctx, 0)
            t0 = time.perf_counter()
            keys = g.get_slots(G["key_slots"][rows])
            present = keys.reshape(-1, 32).any(axis=1)
            vals = np.repeat(fsids.reshape(-1, 32), nkeys[fin], axis=0)
            a.put(0, keys.reshape(-1, 32)[present], vals[present])
            r.put(fsids, sizes)
            host.append(1e3 * (time.perf_counter() - t0))
            assert (a.count(0)[0], r.stats().objects) == on_device
            a.close()
            r.close()
        out["write_%d" % B] = {"finished": int(len(fin)), "keys_put": puts, "cache_write_ms": stat(dev[1:]),
                               "host_gather_put_ms": stat(host[1:])}
        d_f.free()
        d_s.free()
    return out


def main():
    name = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = capi.Context(0, host_threads=0)
    out = {"reps": reps, "command": "python tools/cwrite_probe.py " + " ".join(sys.argv[1:])}
    if len(sys.argv) > 3 and sys.argv[3] == "write":
        S = int(sys.argv[4]) if len(sys.argv) > 4 else 22075
        P = int(sys.argv[5]) if len(sys.argv) > 5 else 32
        out["cache_write"] = write_probe(ctx, reps, S, P)
    else:
        out["a"] = shape(ctx, "a", Flat(100_000, 1, one_dot=True), reps)
        out["b"] = shape(ctx, "b", Flat(1_000, 1_000), reps)
        out["c"] = shape(ctx, "c", Flat(1, 100_000), reps)
    ctx.close()
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
