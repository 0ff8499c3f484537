"""One-launch closed loop for the rigid vehicles on the v1 tasks and the multi-waypoint v2 task (amenv_rigid_policy.hpp), with and without
the observation normaliser inside the launch (amenv_rollout_policy_norm): the env part replays bit for bit through amenv_step's lane
kernel, the normalised rows are bit-identical to amenv_obsnorm_apply under the entry statistics, the statistics merge the raw rows 1..T,
PPO on the v1 task runs it end to end, and the configurations it is not built for are refused."""
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import PPO, ActorCritic
from tests.switch_harness import buffers as _buffers, policy as _policy
from tests.test_gpu_ppo import gae_magnitude
from tests.test_rollout_v1_cpu import RunningMeanStd

pytestmark = pytest.mark.gpu


def _env(vehicle, task, nwp, n, **kw):
    return amd.GpuWaypointEnv(n, vehicle=vehicle, task=task, num_waypoints=nwp, seed=4, max_episode_steps=60, **kw)


# sizes: 300 and 4096 run the 16-env workgroups, 12000 the 64-env ones, 40000 the 128-env ones (AMENV_RIGID_WG16_MAX / WG64_MAX)
@pytest.mark.parametrize("vehicle,task,nwp,n", [("quad", "v1_scaled", 1, 300), ("quad", "v1_raw", 1, 4096), ("hexa", "v1_raw", 1, 40000),
                                                ("quad", "v2", 3, 12000)])
def test_rigid_lane_closed_loop_replays_bit_for_bit(vehicle, task, nwp, n):
    """amenv_rollout_policy on the configs the lane-quad form does not serve: replaying the recorded clipped actions through amenv_step on a
    lane-kernel handle reproduces every observation / reward / done / info row, the terminal rows where done, the final state and the Monitor
    totals bit for bit; the policy part against the fp32 modules (bf16 tolerance), the noise statistically, determinism."""
    T = 96
    env = _env(vehicle, task, nwp, n)
    ref = _env(vehicle, task, nwp, n, kernel="lane")
    assert "step_kernel<" in ref.kernel_name
    od = env.obs_dim
    assert od == (17 if task != "v2" else 20)
    pol = _policy(od)
    o0 = env.reset().clone(); ref.reset()
    dev = env.device
    b = _buffers(T, n, od, dev)
    info = torch.zeros(T, n, dtype=torch.int32, device=dev); tobs = torch.full((T, n, od), float("nan"), device=dev)
    env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, info_bits=info, terminal_obs=tobs, **b)
    torch.cuda.synchronize()
    assert torch.equal(b["obs"][0], o0)
    lo, hi = pol.action_low, pol.action_high
    for t in range(T):
        o, r, d, i = ref.step(torch.max(torch.min(b["actions"][t], hi), lo))
        assert torch.equal(o, b["obs"][t + 1]) and torch.equal(r, b["rewards"][t]) and torch.equal(d, b["dones"][t]) and torch.equal(i, info[t]), t
        dn = d.bool()
        if bool(dn.any()):
            assert torch.equal(ref.terminal_obs[dn], tobs[t][dn]), t
    f1, i1 = env.get_state(); f2, i2 = ref.get_state()
    assert torch.equal(f1, f2) and torch.equal(i1, i2)
    s1, s2 = env.stats(), ref.stats()
    assert s1 == s2 and s1["episodes"] == int(b["dones"].sum()) > n // 2, (s1, s2)
    assert bool(torch.isnan(tobs[~b["dones"].bool()]).all())
    with torch.no_grad():
        flat = b["obs"][:T].reshape(T * n, od)
        mean32 = pol.action_net(pol.mlp_extractor.policy_net(flat)); v32 = pol.value_net(pol.mlp_extractor.value_net(flat)).reshape(-1)
    std = torch.exp(pol.log_std.detach())
    assert float((b["values"].reshape(-1) - v32).abs().max()) < 3e-2 * max(1.0, float(v32.abs().max()))
    z = (b["actions"].reshape(T * n, 4) - mean32) / std
    assert abs(float(z.mean())) < 0.03 and abs(float(z.var()) - 1.0) < 0.04 and float(z.abs().max()) < 6.5
    assert float((torch.corrcoef(z[:50000].T) - torch.eye(4, device=dev)).abs().max()) < 0.04
    lp32 = (-0.5 * z * z - pol.log_std.detach() - 0.9189385332).sum(1)
    assert float((b["logp"].reshape(-1) - lp32).abs().max()) < 0.5 and float((b["logp"].reshape(-1) - lp32).abs().mean()) < 0.05
    env2 = _env(vehicle, task, nwp, n); env2.reset()
    b2 = _buffers(T, n, od, dev)
    env2.rollout_policy(pol.flat_param, T, seed=77, draw0=5, **b2)
    assert all(torch.equal(b2[k], b[k]) for k in b)
    env.close(); ref.close(); env2.close()


@pytest.mark.parametrize("vehicle,task,n", [("quad", "v1_raw", 4096), ("hexa", "v2", 20000)])
def test_normaliser_inside_the_launch(vehicle, task, n):
    """amenv_rollout_policy_norm: every buffer row and terminal row is ObsNormalizer.normalize(raw) under the ENTRY statistics, bit for bit
    (raw rows from a lane-kernel replay); afterwards the statistics are a sequential RunningMeanStd over the raw rows 1..T (fp64 rounding),
    count = count0 + T n exactly; update=False leaves them bit-identical."""
    T = 64
    env = _env(vehicle, task, 1, n)
    od = env.obs_dim
    pol = _policy(od)
    norm = ObsNormalizer(od)
    norm.update(env.reset())
    dev = env.device
    b = _buffers(T, n, od, dev)
    env.rollout_policy(pol.flat_param, T, seed=5, draw0=0, obs_normalizer=norm, **b)        # warm-up: non-trivial statistics
    mean0, var0, count0 = norm.get()
    assert count0 == (1e-4 + n) + T * n
    entry = ObsNormalizer(od); entry.set(mean0, var0, count0)
    ref = _env(vehicle, task, 1, n, kernel="lane"); ref.reset()
    f, i = env.get_state(); ref.set_state(f, i)
    raw = torch.zeros(T + 1, n, od, device=dev)
    raw[0] = ref.observe()
    info = torch.zeros(T, n, dtype=torch.int32, device=dev); tobs = torch.full((T, n, od), float("nan"), device=dev)
    env.rollout_policy(pol.flat_param, T, seed=5, draw0=T, info_bits=info, terminal_obs=tobs, obs_normalizer=norm, **b)
    torch.cuda.synchronize()
    assert torch.equal(b["obs"][0], entry.normalize(raw[0]))
    lo, hi = pol.action_low, pol.action_high
    for t in range(T):
        o, r, d, _ = ref.step(torch.max(torch.min(b["actions"][t], hi), lo))
        raw[t + 1] = o
        assert torch.equal(entry.normalize(o), b["obs"][t + 1]) and torch.equal(r, b["rewards"][t]) and torch.equal(d, b["dones"][t]), t
        dn = d.bool()
        if bool(dn.any()):
            assert torch.equal(entry.normalize(ref.terminal_obs[dn]), tobs[t][dn]), t
    assert int(b["dones"].sum()) > n // 2 and float(b["obs"].abs().max()) <= norm.clip_obs
    mean1, var1, count1 = norm.get()
    rms = RunningMeanStd(od)
    rms.mean, rms.var, rms.count = mean0.copy(), var0.copy(), count0
    rows = raw.cpu().numpy().astype(np.float64)
    for t in range(1, T + 1):
        rms.update(rows[t])
    assert count1 == count0 + T * n
    np.testing.assert_allclose(mean1, rms.mean, rtol=1e-10, atol=1e-12)
    # (the sum-of-squares moments lose |mean|^2 / var digits on near-constant columns, as amenv_obsnorm_update's do)
    np.testing.assert_allclose(var1, rms.var, rtol=1e-10, atol=1e-14 * float(np.max(rms.mean ** 2 + rms.var)))
    # evaluation: update=False leaves the statistics bit-identical, the rows are still normalised with them
    b3 = _buffers(T, n, od, dev)
    env.rollout_policy(pol.flat_param, T, seed=5, draw0=2 * T, obs_normalizer=norm, update_normalizer=False, **b3)
    mean2, var2, count2 = norm.get()
    assert np.array_equal(mean2, mean1) and np.array_equal(var2, var1) and count2 == count1
    assert float(b3["obs"].abs().max()) <= norm.clip_obs
    env.close(); ref.close(); norm.close(); entry.close()


def test_ppo_fused_rollout_with_normaliser_on_the_v1_task():
    """PPO(GpuWaypointEnv(task="v1_raw"), obs_normalizer=ObsNormalizer(17), fused_rollout=True): two iterations; the buffer is consistent
    (GAE recomputed from its own rewards / values / dones), losses finite, the normaliser has counted the reset rows once and 2 T n rows."""
    n, T = 4096, 64
    env = amd.GpuWaypointEnv(n, task="v1_raw", seed=2, max_episode_steps=40)
    norm = ObsNormalizer(17)
    algo = PPO(env, obs_normalizer=norm, fused_rollout=True, n_steps=T, n_epochs=2, batch_size=8192, seed=1)
    algo.learn(2 * T * n)
    assert len(algo.log) == 2 and algo.num_timesteps == 2 * T * n
    assert all(math.isfinite(x) for rec in algo.log for x in rec.values())
    _, _, count = norm.get()
    assert count == ((1e-4 + n) + T * n) + T * n
    b = algo.buffer
    r, v, dn, lv = (x.cpu().numpy() for x in (b.rewards, b.values, b.dones, b.last_values))
    adv_ref, _ = O.gae_reference(r, v, dn, lv, algo.gamma, algo.gae_lambda)
    assert (np.abs(b.advantages.cpu().numpy() - adv_ref) / (1.0 + gae_magnitude(r, v, dn, lv, algo.gamma, algo.gae_lambda))).max() < 1e-6
    assert float(b.obs.abs().max()) <= norm.clip_obs and int(b.dones.sum()) > 0
    env.close(); norm.close()


def test_refusals():
    """Arm + fused rollout + normaliser (PPO), a normaliser of another dim, an fp64 env, a closed normaliser: AmenvError, nothing launched."""
    arm = amd.GpuWaypointEnv(64, vehicle="hexa_arm", seed=1)
    with pytest.raises(L.AmenvError):
        PPO(arm, obs_normalizer=ObsNormalizer(arm.obs_dim), fused_rollout=True, n_steps=8)
    arm.close()
    T, n = 4, 64
    env = amd.GpuWaypointEnv(n, task="v1_raw", seed=1)
    env.reset()
    pol = ActorCritic(17, 4).cuda().flatten_()
    b = _buffers(T, n, 17, env.device)
    wrong = ObsNormalizer(20)
    with pytest.raises(L.AmenvError, match="obs_dim"):
        env.rollout_policy(pol.flat_param, T, 0, 0, obs_normalizer=wrong, **b)
    closed = ObsNormalizer(17); closed.close()
    with pytest.raises(L.AmenvError, match="non-NULL"):
        env.rollout_policy(pol.flat_param, T, 0, 0, obs_normalizer=closed, **b)
    env.close(); wrong.close()
    f64 = amd.GpuWaypointEnv(n, task="v1_raw", seed=1, dtype="f64")
    f64.reset()
    norm = ObsNormalizer(17)
    for kw in ({}, {"obs_normalizer": norm}):
        with pytest.raises(L.AmenvError):
            f64.rollout_policy(pol.flat_param, T, 0, 0, **kw, **b)
    f64.close(); norm.close()
