"""bench.py's command line: the result line is written whole whatever the
pipe does, --dump-outputs writes the File IDs as float32 rows, and a plain run
(no --full) on a small configs[1]-distributed set prints one compact line,
honours --steps, and dumps exactly the oracle's File IDs of the seeded set."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from reflow_amd.workloads import GiB, c2_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_SEED = 0x5EED0002


def test_write_all_drains_a_full_nonblocking_pipe():
    import bench
    data = os.urandom(1 << 20)  # far more than a pipe holds
    r, w = os.pipe()
    os.set_blocking(w, False)
    got = []

    def reader():
        while True:
            b = os.read(r, 4096)
            if not b:
                return
            got.append(b)

    t = threading.Thread(target=reader)
    t.start()
    bench.write_all(w, data)
    os.close(w)
    t.join()
    os.close(r)
    assert b"".join(got) == data


def test_dump_outputs_writes_float32_rows(tmp_path):
    import bench

    class One:
        world, rank = 1, 0

    class Second:
        world, rank = 2, 1

    ids = np.arange(5 * 32, dtype=np.uint8).reshape(5, 32)
    d = tmp_path / "a" / "b"  # created on demand
    bench.dump_outputs(str(d), One, {"_digests": ids})
    bench.dump_outputs(str(d), Second, {"_digests": ids[::-1]})
    assert sorted(os.listdir(d)) == ["file_ids.npy", "file_ids_rank1.npy"]
    got = np.load(d / "file_ids.npy")
    assert got.dtype == np.float32 and got.shape == (5, 32) and (got == ids).all()
    assert (np.load(d / "file_ids_rank1.npy") == ids[::-1]).all()


@pytest.mark.gpu
def test_gpu_plain_run_line_and_dump(oracle, tmp_path):
    import bench
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}  # one rank
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--sha-gib", "0.25", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert (d["steps"], d["warmup"], d["full"], d["n_gpus"]) == (3, 1, False, 1)
    assert (d["unit"], d["higher_is_better"], d["dtype"]) == ("GB/s", True, "u32")
    assert not set(bench.FULL_KEYS) & set(d)  # no secondary section ran
    lens = c2_sizes(total_bytes=int(0.25 * GiB), seed=C2_SEED)
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(float(lens.sum()) / (d["ms_per_step"] * 1e-3) / 1e9, rel=2e-3)
    want = np.zeros((len(lens), 32), dtype=np.uint8)
    oracle.lib().orc_stream_sha256_batch(C2_SEED, lens.ctypes.data, len(lens), want.ctypes.data,
                                         min(16, os.cpu_count() or 1))
    got = np.load(out / "file_ids.npy")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert (got == want).all()
