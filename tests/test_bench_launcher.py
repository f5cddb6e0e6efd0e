"""bench.py's own launcher (`python bench.py --gpus N` without a torchrun environment), exercised without a GPU:
DQP_BENCH_DRY_RUN=1 stops every rank after the rendezvous (gloo) and before any GPU call."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(DQP_BENCH_DRY_RUN="1", **env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)


def test_gpus_2_starts_two_ranks_and_prints_one_line():
    r = run(["--gpus", "2", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["steps"] == 3 and d["scaling"] == "weak"


def test_config_4_is_strong_scaling_and_single_rank_needs_no_launcher():
    r = run(["--config", "4"])
    assert r.returncode == 0, r.stderr
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["config"] == 4


def test_child_failure_fails_the_parent():
    r = run(["--gpus", "2"], DQP_BENCH_DRY_RUN_FAIL_RANK="1")
    assert r.returncode != 0


def test_world_size_mismatch_is_an_error():
    r = run(["--gpus", "4"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_dump_outputs_writes_float64_within_the_cap_on_a_fixed_sample(tmp_path):
    """--dump-outputs on a CPU stand-in workload over the 64 MiB cap: every batch-major array keeps the same rows
    (a seeded sample, in batch order), other arrays are written whole, and two runs write identical files."""
    import numpy as np
    import torch
    import bench

    B = 4096

    class Stub:
        def outputs(self):
            row = torch.arange(B, dtype=torch.int32)
            big = row[:, None].double().repeat(1, 2100)                  # 68.8 MB alone
            return {"row": row, "big": big}, {"loss": torch.tensor([0.5], dtype=torch.float32)}

    rows = []
    for d in ("a", "b"):
        rows.append(bench.dump_outputs(torch, Stub(), str(tmp_path / d)))
    assert rows[0] == rows[1] < B
    total = 0
    for name in ("row", "big", "loss"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
    row, big = np.load(tmp_path / "a" / "row.npy"), np.load(tmp_path / "a" / "big.npy")
    assert row.shape == (rows[0],) and big.shape == (rows[0], 2100)
    assert np.all(np.diff(row) > 0) and np.array_equal(big[:, 0], row) and np.array_equal(big[:, -1], row)
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.5]
