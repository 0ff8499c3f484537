"""bench.py --dump-outputs on the GPU: the files hold what the last timed step returned -- the same steps replayed here give the same
arrays bit for bit -- and the same arguments give the same files on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP, REPEATS, PREROLL = 4096, 100, 7, 2, 300
NAMES = ["obs", "reward", "done", "info_bits", "terminal_obs", "ep_return", "ep_len"]


def _bench(out_dir, mode):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--repeats", str(REPEATS),
           "--preroll", str(PREROLL), "--envs-per-gpu", str(N), "--mode", mode, "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["windows"]["count"] == REPEATS and line["ms_per_step"] > 0
    assert line["dump_outputs"]["rows"] == line["dump_outputs"]["of_rows"] == N
    assert line["dump_outputs"]["files"] == sorted(k + ".npy" for k in NAMES)
    return {k: np.load(os.path.join(out_dir, k + ".npy")) for k in NAMES}


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    import rl_aerial_manipulator_amd as amd

    eager = _bench(tmp_path / "eager", "eager")
    # eager mode steps exactly preroll, warm-up, then --repeats windows of --steps steps, each run starting at the ring's first batch
    env = amd.GpuWaypointEnv(N, device=0, vehicle="hexa_arm", seed=0)
    env.reset()
    ring = bench.make_actions(torch, "hover", N, bench.GRAPH_CHUNK, torch.device("cuda", 0), seed=1234, act_dim=env.act_dim)
    for k in [PREROLL, WARMUP] + [STEPS] * REPEATS:
        for t in range(k):
            env.step(ring[t % bench.GRAPH_CHUNK])
    torch.cuda.synchronize()
    here = bench.step_outputs(env)
    env.close()
    for k in NAMES:
        assert eager[k].dtype == (np.float32 if here[k].dtype == np.float32 else np.float64), k
        assert eager[k].shape == here[k].shape and np.array_equal(eager[k], here[k].astype(eager[k].dtype)), k
    assert eager["obs"].shape == (N, 29) and np.isfinite(eager["obs"]).all() and np.isfinite(eager["reward"]).all()
    done = eager["done"] != 0
    info = eager["info_bits"].astype(np.int64)
    assert np.array_equal(done, (info & (amd._lib.INFO_TERMINATED | amd._lib.INFO_TRUNCATED)) != 0)
    assert np.all(eager["terminal_obs"][~done] == 0) and np.all(eager["ep_len"][done] > 0)

    # graph mode (the default), twice: identical files
    a, b = _bench(tmp_path / "graph_a", "graph"), _bench(tmp_path / "graph_b", "graph")
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
