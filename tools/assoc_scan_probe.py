"""Times one rf_assoc_scan_device and one rf_assoc_compact of a large table
with rf_timer_* (the record in DESIGN.md §K5 "scan"): N live keys (default
1e7) in a table of 2 * CAPACITY slots (default CAPACITY = 2^24), no deleted
keys.  Prints one JSON line.

    python tools/assoc_scan_probe.py [N] [CAPACITY]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflow_amd import capi  # noqa: E402


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    capacity = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 24
    ctx = capi.Context(0, host_threads=0)
    a = capi.Assoc(ctx, capacity=capacity)
    rng = np.random.default_rng(1)
    step = 2_500_000
    for lo in range(0, n, step):
        m = min(step, n - lo)
        keys = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        assert (a.put(lo // step % 2, keys, keys | 1) == 0).all()
    occupied, slots = a.stats()
    live, deleted = a.count()
    dk, dv = capi.DeviceBuffer(ctx, 32 * live), capi.DeviceBuffer(ctx, 32 * live)
    dkd, dn = capi.DeviceBuffer(ctx, 4 * live), capi.DeviceBuffer(ctx, 8)
    scan_ms = []
    for _ in range(5):
        ctx.sync()
        ctx.timer_start()
        a.scan_device(-1, live, dk.ptr, dv.ptr, dkd.ptr, dn.ptr)
        scan_ms.append(ctx.timer_stop())
    assert int(dn.to_numpy(np.uint64)[0]) == live
    compact_ms, compact_wall_ms = [], []
    for _ in range(3):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        a.compact(capacity)
        compact_ms.append(ctx.timer_stop())
        compact_wall_ms.append(1e3 * (time.perf_counter() - t0))
    assert a.stats() == (live, slots)
    # the byte model of DESIGN.md: the scan reads the tags, the occupied
    # slots' values, and the live bits, values, keys and tags again for the
    # entries it writes
    scan_bytes = 4 * slots + 32 * occupied + 2 * (slots // 8) + (32 + 32 + 4) * live + 68 * live
    best = min(scan_ms)
    print(json.dumps({
        "live": live, "deleted": deleted, "slots": slots, "scan_ms": [round(x, 3) for x in scan_ms],
        "scan_model_bytes": scan_bytes, "scan_model_GBps": round(scan_bytes / best / 1e6, 1),
        "compact_ms": [round(x, 3) for x in compact_ms], "compact_wall_ms": [round(x, 3) for x in compact_wall_ms],
    }))


if __name__ == "__main__":
    main()
