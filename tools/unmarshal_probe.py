"""Times the unmarshal of Fileset JSON (DESIGN.md §5 "Unmarshal"): the step of
Eval.lookup between the plan and missing(), on the three shapes of
tools/cwrite_probe.py:

    a   10^5 values of one file "."
    b   10^3 values of 10^3 files
    c   one value of 10^5 files

The documents are the arena rf_fileset_marshal_device leaves in HBM.  Timed, per
shape, REPS runs after one warm-up, host clock around each call:

    device   rf_fileset_unmarshal_device over that arena (the call ends in a
             synchronise), split as rf_fileset_forest_times gives it
    host     rf_fileset_unmarshal_flat on 16 threads over the same bytes on the
             host (the sequential form alone, no per-byte check beside it)
    python   json.loads of every document plus a flatten into (ID, Size) rows --
             an outside reference, one run

The device rows must equal the host form's.  Writes one JSON record to
profiles/unmarshal/<name>.json and prints it.

    python tools/unmarshal_probe.py NAME [REPS]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cwrite_probe import Flat, stat  # noqa: E402
from reflow_amd import capi  # noqa: E402

OUT_DIR = os.path.join(ROOT, "profiles", "unmarshal")


def loads_rows(docs):
    ids, sizes = [], []

    def walk(o):
        for c in o.get("List", ()):
            walk(c)
        for v in o.get("Fileset", {}).values():
            ids.append(bytes.fromhex(v["ID"][7:]))
            sizes.append(v["Size"])
    for d in docs:
        walk(json.loads(d))
    return ids, sizes


def shape(ctx, name, flat, reps):
    L = capi.lib()
    n = flat.n
    d_ids = ctx.upload(flat.keep["ids"])
    no_ids = capi.FilesetTree(flat.tree.n_nodes, flat.tree.list_ptr, flat.tree.list_child, flat.tree.entry_ptr,
                              flat.tree.paths, flat.tree.path_lens, None, flat.tree.sizes)
    batch = capi.JsonBatch(ctx, tree=no_ids, roots=flat.roots, d_ids32=d_ids.ptr)
    lens = batch.lens()
    arena_bytes = int(((lens + 15) & ~15).sum())
    d_arena, d_offs, d_lens = batch.device()
    dev, parts = [], []
    rows = None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        f = capi.FilesetForest.from_device(ctx, d_arena, arena_bytes, d_offs, d_lens, n)
        dev.append(1e3 * (time.perf_counter() - t0))
        parts.append(f.times())
        assert f.n_accepted == n and f.n_entries == flat.entries, name
        if rows is None:
            s = f.copy()
            rows = s["ids32"].tobytes(), s["sizes"].tobytes()
        f.close()
    docs = batch.copy()
    buf, offs = capi.pack_docs(docs)
    host = []
    for _ in range(reps + 1):
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        capi._check(L.rf_fileset_unmarshal_flat(buf.ctypes.data, offs.ctypes.data, n, 0, 16, ctypes.byref(h)))
        host.append(1e3 * (time.perf_counter() - t0))
        hf = capi.FilesetForest(h)
        s = hf.copy()
        assert (s["ids32"].tobytes(), s["sizes"].tobytes()) == rows, name
        hf.close()
    t0 = time.perf_counter()
    ids, sizes = loads_rows(docs)
    py = 1e3 * (time.perf_counter() - t0)
    assert b"".join(ids) == rows[0] and np.array(sizes, np.int64).tobytes() == rows[1], name
    batch.close()
    d_ids.free()
    cols = list(zip(*parts[1:]))
    return {"values": n, "entries": flat.entries, "json_bytes": int(lens.sum()), "arena_bytes": arena_bytes,
            "device_form_ms": stat(dev[1:]), "host_form_16_threads_ms": stat(host[1:]),
            "python_json_loads_flatten_ms": round(py, 2),
            "device_split_ms": {"upload": stat(cols[0]), "passes_scans_readback": stat(cols[1]),
                                "outputs_scatter": stat(cols[2])},
            "device_slowest_beats_host_fastest": max(dev[1:]) < min(host[1:])}


def main():
    name = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = capi.Context(0, host_threads=0)
    out = {"reps": reps, "command": "python tools/unmarshal_probe.py " + " ".join(sys.argv[1:])}
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
