"""bench.py --dump-outputs / --full (host side: no device is touched).

dump_outputs() writes each array whole when it fits its share of the byte
budget and as a fixed seeded sample otherwise; the same arguments give the
same files, so two builds can be compared output for output."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _dump(tmp, arrays, world=1, rank=0):
    import bench
    args = argparse.Namespace(dump_outputs=str(tmp))
    bench.dump_outputs(args, arrays, rank, world)
    return {f: np.load(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}


def test_dump_small_arrays_whole_and_exact(tmp_path):
    a = torch.arange(-5, 1000, dtype=torch.int32)
    b = torch.tensor([-2**31, 2**31 - 1, 0x01000001], dtype=torch.int32)
    got = _dump(tmp_path, {"a": a, "b": b.reshape(3, 1)})
    assert sorted(got) == ["a.npy", "b.npy"]
    assert got["a.npy"].dtype == np.float64 and got["b.npy"].dtype == np.float64
    # float64 holds every 32-bit record exactly
    assert np.array_equal(got["a.npy"], a.numpy().astype(np.float64))
    assert got["b.npy"].tolist() == [-2.0**31, 2.0**31 - 1, float(0x01000001)]


def test_dump_large_array_is_fixed_sample_within_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 1000)  # 1000 elements in all
    big = torch.arange(100_000, dtype=torch.int32)
    small = torch.arange(7, dtype=torch.int32)
    one = _dump(tmp_path / "one", {"big": big, "small": small})
    two = _dump(tmp_path / "two", {"big": big, "small": small})
    assert one["big.npy"].shape == (500,) and one["small.npy"].shape == (7,)
    assert sum(v.nbytes for v in one.values()) <= 8 * 1000
    assert all(np.array_equal(one[k], two[k]) for k in one)
    # a sample of the array itself, at sorted positions spread over all of it
    s = one["big.npy"]
    assert np.all(np.diff(s) >= 0) and s.min() < 10_000 and s.max() > 90_000
    # another output at one sampled position shows in the dump
    changed = big.clone()
    changed[int(s[250])] = -1
    three = _dump(tmp_path / "three", {"big": changed, "small": small})
    assert not np.array_equal(three["big.npy"], s)


def test_dump_names_carry_rank_when_sharded(tmp_path):
    got = _dump(tmp_path, {"x": torch.zeros(4, dtype=torch.int32)}, world=2, rank=1)
    assert list(got) == ["x_rank1.npy"]


def test_bench_options_parse_without_gpu():
    """--full and --dump-outputs exist; a dump of a config other than the
    headline is refused before anything touches the GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--full", "--config", "c2", "--dump-outputs", "x"],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 2 and "unrecognized" not in r.stderr
    assert "--dump-outputs writes the headline" in r.stderr
