#!/usr/bin/env python3
"""Per-step view of the K1 hybrid plan on configs[1], as bench.py runs it
(all-host calibration runs, then the hybrid plan, warm-up, timed steps): one
line per timed step with the legs' times and the prefix hand-over's counters
(rf_sha_plan_prefix_stats), then a JSON summary.

    python tools/prefix_steps.py [--steps 20] [--warmup 5] [--flags 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reflow_amd import capi  # noqa: E402
from reflow_amd.workloads import GiB, arena_layout, c2_sizes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--flags", type=int, default=0)
    args = ap.parse_args()
    ctx = capi.Context(0)
    lens = c2_sizes(total_bytes=64 * GiB, seed=0x5EED0002)
    offs, total = arena_layout(lens)
    arena, out = ctx.alloc(total), ctx.alloc(32 * len(lens))
    d_offs, d_lens = ctx.upload(offs), ctx.upload(lens)
    ctx.gen_fill(arena.ptr, d_offs.ptr, d_lens.ptr, len(lens), 0x5EED0002, total)
    ctx.sync()
    pa = ctx.sha_plan(offs, lens, capi.RF_SHA_ALL_HOST)
    for _ in range(3):
        pa.run(arena.ptr, out.ptr)
        pa.stats()
    pa.close()
    plan = ctx.sha_plan(offs, lens, args.flags)
    st, ps = plan.stats(), plan.prefix_stats()
    print("split: %d host (%d lone), %d duo, %d lane; %d prefixed, %.3f GB planned; feed %.2f GB/s"
          % (st.n_host, ps.n_lone, st.n_solo, len(lens) - st.n_host - st.n_solo, ps.n_prefixed,
             ps.planned_bytes / 1e9, ctx.host_link()[0] / 1e9))
    rows = []
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        plan.run(arena.ptr, out.ptr)
        s, p = plan.stats(), plan.prefix_stats()
        wall = (time.perf_counter() - t0) * 1e3
        if i < args.warmup:
            continue
        rows.append((wall, s.last_ms_host, s.last_ms_solo, s.last_ms_lanes, p.taken, p.missed, p.skipped_bytes))
        # the host leg's feed: the bytes that crossed the link over its wall time
        feed = (st.host_bytes - p.skipped_bytes) / (s.last_ms_host * 1e-3) / 1e9 if s.last_ms_host > 0 else 0.0
        print("step %2d: wall %7.1f ms, host %7.1f, solo %7.1f, lanes %5.1f; taken %d missed %d, "
              "%.3f of %.3f GB planned skipped; host feed %.2f GB/s"
              % (i - args.warmup, wall, s.last_ms_host, s.last_ms_solo, s.last_ms_lanes, p.taken, p.missed,
                 p.skipped_bytes / 1e9, p.planned_bytes / 1e9, feed))
    r = np.array(rows, dtype=np.float64)
    print(json.dumps({"steps": len(rows), "wall_ms_mean": round(float(r[:, 0].mean()), 2),
                      "host_ms_mean": round(float(r[:, 1].mean()), 2), "solo_ms_mean": round(float(r[:, 2].mean()), 2),
                      "solo_le_host_every_step": bool((r[:, 2] <= r[:, 1]).all()),
                      "taken": int(r[:, 4].sum()), "missed": int(r[:, 5].sum()),
                      "skipped_gb_mean": round(float(r[:, 6].mean()) / 1e9, 3),
                      "skipped_gb_min": round(float(r[:, 6].min()) / 1e9, 3),
                      "skipped_gb_max": round(float(r[:, 6].max()) / 1e9, 3),
                      "planned_gb": round(ps.planned_bytes / 1e9, 3),
                      "n_prefixed": int(ps.n_prefixed), "n_lone": int(ps.n_lone), "host_bytes_gb": round(st.host_bytes / 1e9, 3)}))
    plan.close()


if __name__ == "__main__":
    main()
