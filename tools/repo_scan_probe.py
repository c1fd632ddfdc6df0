"""Times the repository index's read-back calls (rf_repo_scan_device,
rf_repo_collect_list / _device, rf_repo_compact, rf_repo_save, rf_repo_restore)
at the size the assoc's scan figures use: N objects (default 10^7) in the
table rf_repo_new(N) gives (2^25 slots), beside what the library offered
before for "collect and know what went" (the record in DESIGN.md §5
"Repository index: listing and persistence").

Per repetition, alternating, after one warm-up round (the index holds all N
objects at the start of each step; what a step removed is Put back, untimed):

    scan_device          every live object's ID and size into device arrays
    collect_list_device  keeping a seeded half (a filter built by rf_bloom_new +
                         rf_bloom_add): the removed IDs and sizes stay on the device
    compact              right after it, over the N / 2 tombstones, min_capacity N
    collect_list         the host form: the removed IDs and sizes in host arrays
    baseline             the caller's host-resident array of every ID through
                         rf_bloom_collect (dead indices), then rf_repo_remove of
                         the dead -- the same knowledge on the host (gathering the
                         dead IDs for the remove is left out of its time)
    save, restore        the file of N objects (40 N bytes and its checksums)

Device events (torch.cuda.Event on the context's stream) go around the device
forms and compact; a host clock goes around everything, each call ending in a
device synchronise.  The calls that return when applied (collect_list_device,
compact) read their counters back inside, so their event time includes that
round trip.  Median, min and max of REPS.  The check: the new paths and the
baseline remove the same set, and the restored index scans to the saved one.
Prints one JSON line; OUT (optional) also gets it.

    python tools/repo_scan_probe.py [N] [REPS] [OUT]
"""
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflow_amd import capi  # noqa: E402


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def first_words(ids):
    """The first 8 bytes of each 32-byte row, sorted: a set's fingerprint."""
    return np.sort(np.ascontiguousarray(ids).reshape(-1, 32)[:, :8].copy().view(np.uint64).reshape(-1))


def main():
    N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 7
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    ctx = capi.Context(0)  # the default host pool: save sorts and hashes on it
    stream = torch.cuda.ExternalStream(ctx.stream)

    def timed(fn):
        """(event ms, wall ms) of fn(), which leaves its work on the context's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        return r, 1e3 * (time.perf_counter() - t0)

    rng = np.random.default_rng(14)
    ids = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    sizes = rng.integers(0, 1 << 30, size=N).astype(np.int64)
    keep = np.sort(np.random.default_rng(15).permutation(N)[:N // 2])
    repo = capi.Repo(ctx, capacity=N)
    assert (repo.put(ids, sizes) == 0).all()
    m, k = capi.bloom_estimate(max(N // 2, 1), 0.01)
    bloom = capi.Bloom.new(ctx, m, k)
    bloom.add(ids[keep])
    d_ids, d_sizes, d_n, d_nb = ctx.alloc(32 * N), ctx.alloc(8 * N), ctx.alloc(8), ctx.alloc(8)
    # the host form's arrays, allocated once as a caller's would be
    h_ids, h_sizes = np.zeros((N, 32), np.uint8), np.zeros(N, np.int64)
    h_cnt, h_bytes = ctypes.c_uint64(), ctypes.c_int64()

    def host_collect_list():
        rc = capi.lib().rf_repo_collect_list(repo._h, bloom._h, N, h_ids.ctypes.data, h_sizes.ctypes.data,
                                             ctypes.byref(h_cnt), ctypes.byref(h_bytes))
        assert rc == capi.RF_OK, rc

    fd, path = tempfile.mkstemp(suffix=".rfrepo")
    os.close(fd)

    def put_back(dead_ids, dead_sizes):
        assert (repo.put(dead_ids, dead_sizes) == 0).all()
        assert repo.stats().objects == N

    ms = {k_: [] for k_ in ("scan_device_event", "scan_device_wall", "collect_list_device_event",
                            "collect_list_device_wall", "compact_event", "compact_wall", "collect_list_wall",
                            "baseline_bloom_collect_wall", "baseline_remove_wall", "baseline_wall", "save_wall",
                            "restore_wall")}
    check = {}
    for rep in range(reps + 1):  # the first round is warm-up
        t = {}
        t["scan_device_event"], t["scan_device_wall"] = timed(
            lambda: repo.scan_device(N, d_ids.ptr, d_sizes.ptr, d_n.ptr, stream=ctx.stream))
        assert int(d_n.to_numpy(np.uint64)[0]) == N
        # the new path, device form; then compact over its tombstones
        t["collect_list_device_event"], t["collect_list_device_wall"] = timed(
            lambda: repo.collect_list_device(bloom, N, d_ids.ptr, d_sizes.ptr, d_n.ptr, d_nb.ptr, stream=ctx.stream))
        n_dead = int(d_n.to_numpy(np.uint64)[0])
        dev_dead_ids = d_ids.to_numpy(np.uint8, count=32 * n_dead).reshape(-1, 32)
        dev_dead_sizes = d_sizes.to_numpy(np.int64, count=n_dead)
        st = repo.stats()
        assert (st.objects, st.tombstones) == (N - n_dead, n_dead)
        t["compact_event"], t["compact_wall"] = timed(lambda: repo.compact(N))
        st = repo.stats()
        assert (st.objects, st.tombstones, st.capacity) == (N - n_dead, 0, check.get("capacity", st.capacity))
        check["capacity"] = int(st.capacity)
        put_back(dev_dead_ids, dev_dead_sizes)
        # the new path, host form
        _, t["collect_list_wall"] = wall(host_collect_list)
        h_n, h_nb = h_cnt.value, h_bytes.value
        put_back(h_ids[:h_n], h_sizes[:h_n])
        # what the library offered before: the caller's own array of every ID
        (dead_idx, dead_bytes), t["baseline_bloom_collect_wall"] = wall(lambda: bloom.collect(ids, sizes))
        b_ids = ids[dead_idx]  # (the gather is not timed: in the baseline's favour)
        removed, t["baseline_remove_wall"] = wall(lambda: repo.remove(b_ids))
        t["baseline_wall"] = t["baseline_bloom_collect_wall"] + t["baseline_remove_wall"]
        assert removed.all() and repo.stats().objects == N - len(dead_idx)
        put_back(b_ids, sizes[dead_idx])
        # the same set every way
        want = first_words(b_ids)
        assert n_dead == h_n == len(dead_idx) and h_nb == dead_bytes == int(d_nb.to_numpy(np.int64)[0])
        assert (first_words(dev_dead_ids) == want).all() and (first_words(h_ids[:h_n]) == want).all()
        check.update(dead=n_dead, dead_bytes=int(dead_bytes))
        _, t["save_wall"] = wall(lambda: repo.save(path))
        restored, t["restore_wall"] = wall(lambda: capi.Repo.restore(ctx, path))
        if rep == reps:  # the restored index scans to the saved one
            r_ids, r_sizes, r_n, _ = restored.scan()
            assert r_n == N and (first_words(r_ids) == first_words(ids)).all() and int(r_sizes.sum()) == int(sizes.sum())
            check["file_bytes"] = os.path.getsize(path)
        restored.close()
        if rep:
            for k_, v in t.items():
                ms[k_].append(v)
    os.unlink(path)
    st = repo.stats()
    out = {"objects": N, "capacity": int(st.capacity), "reps": reps, "device_bytes": int(st.device_bytes),
           "bloom": {"m": int(m), "k": int(k)}, "check": check, "ms": {k_: spread(v) for k_, v in ms.items()}}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    for b in (d_ids, d_sizes, d_n, d_nb):
        b.free()
    bloom.close()
    repo.close()
    ctx.close()


if __name__ == "__main__":
    main()
