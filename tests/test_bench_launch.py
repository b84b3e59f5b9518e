"""bench.py's own N-rank launch (CPU, gloo): `python bench.py --gpus N` without WORLD_SIZE starts N ranks through torch.distributed.run, as the
driver's launcher would, and relays rank 0's line and the exit code.  --launch-check stops after the rendezvous, a barrier and an all-gather of the
ranks, before anything touches a GPU (the real N > 1 bench runs on the GPU box: tests/test_gpu_multi_device.py)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_starts_its_own_ranks():
    r = _run(["--gpus", "2", "--backend", "gloo", "--one-device", "--no-cpu-baseline", "--launch-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d == {"launch_check": True, "world": 2, "ranks": [0, 1], "distinct_processes": 2}


def test_a_failing_rank_ends_the_launch_non_zero():
    # WORLD_SIZE set by a launcher but different from --gpus: the rank refuses, and the self-launcher is not entered
    r = _run(["--gpus", "2", "--launch-check"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_dump_outputs_writes_floats_and_samples_above_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: every array as float .npy; above the byte limit the same seeded rows on every run, listed in <name>_rows.npy"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    depth = np.arange(40 * 256, dtype=np.int64).reshape(40, 256) % 4
    had = np.arange(40, dtype=np.int32) * 1000003
    r = bench.dump_outputs(str(tmp_path / "all"), {"depth_maps": (depth.astype(np.uint8), np.float32), "src_hadamard": (had, np.float64)})
    assert r["files"] == ["depth_maps.npy", "src_hadamard.npy"] and not r["sampled"]
    assert np.array_equal(np.load(tmp_path / "all" / "depth_maps.npy"), depth.astype(np.float32))
    assert np.load(tmp_path / "all" / "src_hadamard.npy").dtype == np.float64
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10000)
    runs = []
    for k in range(2):
        d = tmp_path / f"s{k}"
        r = bench.dump_outputs(str(d), {"depth_maps": (depth.astype(np.uint8), np.float32), "src_hadamard": (had, np.float64)})
        assert r["sampled"] and sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 10000 + 4 * 128   # + the .npy headers
        rows = np.load(d / "depth_maps_rows.npy").astype(np.int64)
        assert np.array_equal(np.load(d / "depth_maps.npy"), depth[rows].astype(np.float32))
        runs.append(rows)
    assert np.array_equal(runs[0], runs[1])
