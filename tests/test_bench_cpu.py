"""bench.py's host side without a GPU: the --dump-outputs writer (dtypes, the 64 MB budget, the seeded row sample), the masking of the
episode-end outputs, and the argument checks."""
import os

import numpy as np
import pytest
import torch

import bench


def _arrays(n, obs_dim=29, seed=3):
    r = np.random.RandomState(seed)
    return {"obs": r.randn(n, obs_dim).astype(np.float32), "reward": r.randn(n).astype(np.float32),
            "done": (r.rand(n) < 0.1).astype(np.uint8), "info_bits": r.randint(0, 256, n).astype(np.int32),
            "ep_len": r.randint(0, 1 << 30, n).astype(np.int32)}


def test_dump_outputs_writes_every_array_whole_under_the_budget(tmp_path):
    a = _arrays(4096)
    got = bench.dump_outputs(str(tmp_path), a)
    assert got["rows"] == got["of_rows"] == 4096 and got["files"] == sorted(k + ".npy" for k in a)
    assert not os.path.exists(tmp_path / "env_index.npy")
    for k, v in a.items():
        d = np.load(tmp_path / (k + ".npy"))
        assert d.dtype == (v.dtype if v.dtype == np.float32 else np.float64), k
        assert d.shape == v.shape and np.array_equal(d, v), k       # integers above 2^24 too: float64 holds every int32
    assert got["bytes"] == sum(os.path.getsize(tmp_path / f) for f in got["files"])


def test_dump_outputs_samples_the_same_seeded_rows_from_every_array_over_the_budget(tmp_path):
    a = _arrays(5000)
    budget = 200_000
    got = bench.dump_outputs(str(tmp_path / "x"), a, budget=budget)
    assert got["of_rows"] == 5000 and 0 < got["rows"] < 5000
    assert got["bytes"] <= budget
    rows = np.load(tmp_path / "x" / "env_index.npy")
    assert rows.dtype == np.float64 and rows.shape == (got["rows"],)
    idx = rows.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 5000
    for k, v in a.items():
        assert np.array_equal(np.load(tmp_path / "x" / (k + ".npy")), v[idx]), k
    again = bench.dump_outputs(str(tmp_path / "y"), a, budget=budget)
    assert again["rows"] == got["rows"] and np.array_equal(np.load(tmp_path / "y" / "env_index.npy"), rows)
    # a later dump that fits leaves no stale sample index behind
    bench.dump_outputs(str(tmp_path / "x"), a)
    assert not os.path.exists(tmp_path / "x" / "env_index.npy")


def test_dump_budget_is_64_mb():
    assert bench.DUMP_BUDGET == 64 * 1024 * 1024


def test_step_outputs_zero_the_rows_the_step_did_not_write():
    n, od = 6, 3

    class Env:
        obs = torch.arange(n * od, dtype=torch.float32).reshape(n, od)
        reward = torch.linspace(-1, 1, n)
        done = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.uint8)
        info_bits = torch.tensor([0, 1, 4, 0, 130, 0], dtype=torch.int32)
        terminal_obs = torch.full((n, od), 7.0)
        ep_return = torch.full((n,), 3.5)
        ep_len = torch.full((n,), 11, dtype=torch.int32)

    o = bench.step_outputs(Env())
    assert set(o) == {"obs", "reward", "done", "info_bits", "terminal_obs", "ep_return", "ep_len"}
    for k in ("obs", "reward", "done", "info_bits"):
        assert np.array_equal(o[k], getattr(Env, k).numpy()), k
    d = Env.done.numpy() != 0
    assert np.all(o["terminal_obs"][d] == 7.0) and np.all(o["terminal_obs"][~d] == 0.0)
    assert np.all(o["ep_return"][d] == 3.5) and np.all(o["ep_return"][~d] == 0.0)
    assert np.all(o["ep_len"][d] == 11) and np.all(o["ep_len"][~d] == 0) and o["ep_len"].dtype == np.int32


def test_bench_arguments():
    a = bench.parse(["--steps", "37", "--warmup", "3", "--dump-outputs", "out"])
    assert a.steps == 37 and a.warmup == 3 and a.dump_outputs == "out"
    assert bench.parse([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--dry-run", "--dump-outputs", "out"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)
