"""Per-episode dynamics randomisation of the rigid vehicles (amenv_set_randomization) on the GPU:
{1, 1} ranges change no output bit; the factors are the numpy restatement's (tests/dr_ref.py) and change exactly when an episode does;
the fp64 kernels match the UNCHANGED fp64 oracle given each env's factors as its vehicle; one-launch rollouts and closed loops replay
bit for bit through amenv_step; sharding by env_id_offset and re-keying; refusals leave the state untouched; PPO trains with it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import PPO
from tests import dr_ref
from tests import switch_harness as H

pytestmark = pytest.mark.gpu
SW = H.RANDOMIZATION

DR = amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1))
ONE = amd.DynamicsRandomization()
# (vehicle, task, waypoints): the lane / helper-wave instantiations (KW = 1 v2, KW = 4 v2, KW = 2 v1)
CONFIGS = [("quad", "v2", 1), ("hexa", "v2", 1), ("hexa", "v2", 3), ("quad", "v1_raw", 1)]
_env, _actions = H.make_env, H.actions


# ---- 1. {1, 1} ranges are the identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("vehicle,task,nwp", CONFIGS)
@pytest.mark.parametrize("kernel", ["auto", "lane"])
def test_unit_ranges_are_bit_identical_step_and_rollout(vehicle, task, nwp, dtype, kernel):
    n, T = 300, 40
    a = _env(vehicle, task, nwp, n, dtype=dtype, kernel=kernel)
    b = _env(vehicle, task, nwp, n, dtype=dtype, kernel=kernel, randomization=ONE)
    assert "+dr" in b.kernel_name and "+dr" not in a.kernel_name
    assert torch.equal(a.reset(), b.reset())
    assert torch.equal(b.dynamics_factors(), torch.ones(n, 2 + b.n_rotors, device=b.device))
    H.check_same_steps_and_rollout(a, b, _actions(T, n, 1, a.device))
    a.close(); b.close()


@pytest.mark.parametrize("vehicle,task,nwp,n", [("quad", "v2", 1, 300), ("hexa", "v2", 2, 4096), ("quad", "v1_raw", 1, 12000),
                                                ("hexa", "v1_scaled", 1, 40000)])
def test_unit_ranges_are_bit_identical_closed_loop(vehicle, task, nwp, n):
    """amenv_rollout_policy and amenv_rollout_policy_norm with {1, 1}: the same rows as the one-lane-per-env form without randomisation
    (block_size = 64 keeps the lane-quad form out of the reference handle); 16-, 64- and 128-env workgroups."""
    T = 48
    a = _env(vehicle, task, nwp, n, block_size=64)
    b = _env(vehicle, task, nwp, n, randomization=ONE)
    a.reset(); b.reset()
    pol = H.policy(a.obs_dim)
    H.check_same_closed_loop(a, b, pol, T)
    (ma, va, ca), (mb, vb, cb) = H.check_same_closed_loop(a, b, pol, T, norm=True)
    assert ca == cb
    np.testing.assert_allclose(ma, mb, rtol=1e-10, atol=1e-12); np.testing.assert_allclose(va, vb, rtol=1e-10, atol=1e-12)
    H.same_state(a, b)
    a.close(); b.close()


# ---- 2. the factors are the restatement's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,dtype", [("quad", "f32"), ("hexa", "f64")])
def test_factors_match_restatement_and_follow_episodes(vehicle, dtype):
    n, T = 512, 300
    env = _env(vehicle, "v2", 1, n, seed=21, dtype=dtype, max_episode_steps=40, randomization=DR)
    env.reset()
    nr = env.n_rotors

    def check():
        f = env.dynamics_factors().cpu().numpy()
        ep = env.get_state()[1][L.I_EPISODE].cpu().numpy()
        assert np.array_equal(f, dr_ref.factors_all(21, 0, ep, nr, DR)), "factors differ from the restatement"
        return f, ep

    f0, ep0 = check()
    assert f0.shape == (n, 2 + nr) and len(np.unique(f0[:, 0])) > n // 2
    acts = _actions(T, n, 5, env.device)
    prev_f, prev_ep = f0, ep0
    changed = 0
    for t in range(T):
        env.step(acts[t])
        f = env.dynamics_factors().cpu().numpy()
        ep = env.get_state()[1][L.I_EPISODE].cpu().numpy()
        same = ep == prev_ep
        assert np.array_equal(f[same], prev_f[same]), t                      # constant within an episode
        assert np.all(np.any(f[~same] != prev_f[~same], axis=1)), t           # a new episode, a new vehicle
        changed += int((~same).sum())
        prev_f, prev_ep = f, ep
    assert changed > n
    check()
    env.close()


# ---- 3. fp64 (and fp32) kernels against the per-env oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,dtype,kernel", [("quad", "v2", 1, "f64", "lane"), ("quad", "v2", 1, "f64", "helper"),
                                                           ("hexa", "v2", 3, "f64", "lane"), ("hexa", "v2", 3, "f64", "helper"),
                                                           ("quad", "v1_raw", 1, "f64", "lane"), ("quad", "v1_raw", 1, "f64", "helper"),
                                                           ("quad", "v2", 1, "f32", "auto"), ("hexa", "v2", 3, "f32", "lane")])
def test_kernels_match_the_oracle_with_per_env_vehicles(vehicle, task, nwp, dtype, kernel):
    """Teacher-forced per step: env i's oracle is the unchanged fp64 oracle on dr_ref.oracle_config(cfg, factors of env i's episode);
    actions near +-1 saturate rotors.  fp64 <= 1e-12, fp32 <= 1e-5 relative to max(1, |x|); reset states bit for bit."""
    n, T = 64, 30
    wide = amd.DynamicsRandomization(mass=(0.6, 1.6), inertia=(0.5, 2.0), thrust=(0.8, 1.2))
    env = _env(vehicle, task, nwp, n, seed=8, dtype=dtype, kernel=kernel, max_episode_steps=12, randomization=wide)
    check_against_per_env_oracle(env, dtype, T)
    env.close()


def check_against_per_env_oracle(env, dtype, T):
    """The gate of the test above on a handle with randomisation on (tests/test_gpu_generic_vehicles.py runs it on its vehicles)."""
    n = env.num_envs
    env.reset()
    base = H.oracle_cfg(env)
    acts = _actions(T, n, 6, env.device, wide=True)
    tol = 1e-12 if dtype == "f64" else 1e-5
    worst, ended = 0.0, 0
    for t in range(T):
        f_prev, i_prev = (x.cpu().numpy() for x in env.get_state())
        fac = env.dynamics_factors().cpu().numpy()
        env.step(acts[t])
        f_new, i_new = (x.cpu().numpy().astype(np.float64) for x in env.get_state())
        done = env.done.cpu().numpy()
        a = acts[t].cpu().numpy()
        for i in range(n):
            orc = O.OracleEnv(dr_ref.oracle_config(base, fac[i], gid=i))
            orc.fstate[:, 0] = f_prev[:, i]
            orc.istate[:, 0] = i_prev[:, i]
            out = orc.step(a[i:i + 1])
            if done[i]:
                ended += 1
                if dtype == "f64":
                    assert out["done"][0] == 1 and np.array_equal(orc.fstate[:, 0], f_new[:, i]) and np.array_equal(orc.istate[:, 0], i_new[:, i]), (t, i)
                continue
            if dtype == "f64":
                assert out["done"][0] == 0 and np.array_equal(orc.istate[:, 0], i_new[:, i]), (t, i)
            err = np.abs(orc.fstate[:13, 0] - f_new[:13, i]) / np.maximum(1.0, np.abs(orc.fstate[:13, 0]))
            worst = max(worst, float(err.max()))
    print(f"randomisation gate {env.kernel_name}: state {worst:.3e} (tol {tol:g}), {ended} episode ends")
    assert worst <= tol, worst
    assert ended > 0
    return worst


# ---- 4. one-launch rollout = T steps -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,dtype", [("quad", "v2", 1, "f32"), ("hexa", "v2", 3, "f64"), ("quad", "v1_raw", 1, "f32"),
                                                    ("hexa", "v1_scaled", 1, "f64")])
def test_rollout_equals_steps(vehicle, task, nwp, dtype):
    n, T = 1000, 80
    a = _env(vehicle, task, nwp, n, dtype=dtype, max_episode_steps=25, randomization=DR)
    b = _env(vehicle, task, nwp, n, dtype=dtype, max_episode_steps=25, randomization=DR)
    H.check_rollout_equals_steps(a, b, _actions(T, n, 2, a.device), min_ended=n, side=(SW,))
    a.close(); b.close()


# ---- 5. the closed loop replays bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,n,norm", [("quad", "v2", 1, 4096, False), ("hexa", "v2", 2, 4096, False),
                                                     ("quad", "v1_raw", 1, 4096, True), ("quad", "v2", 1, 40000, False)])
def test_closed_loop_replays_bit_for_bit(vehicle, task, nwp, n, norm):
    T = 64
    env = _env(vehicle, task, nwp, n, randomization=DR)
    ref = _env(vehicle, task, nwp, n, kernel="lane", randomization=DR)
    H.check_closed_loop_replays(env, ref, T, norm=norm).close()


# ---- 6. sharding and re-keying --------------------------------------------------------------------------------------------------
def test_sharding_and_reseed():
    n, T = 512, 60
    whole = _env("hexa", "v2", 1, n, seed=13, max_episode_steps=20, randomization=DR)
    h0 = _env("hexa", "v2", 1, n // 2, seed=13, max_episode_steps=20, randomization=DR)
    h1 = _env("hexa", "v2", 1, n // 2, seed=13, max_episode_steps=20, randomization=DR, env_id_offset=n // 2)
    H.check_two_shards(whole, h0, h1, n // 2, _actions(T, n, 4, whole.device), side=(SW,))
    before = whole.dynamics_factors().clone()
    whole.reseed(14)
    after = whole.dynamics_factors()
    ep = whole.get_state()[1][L.I_EPISODE].cpu().numpy()
    assert not torch.equal(before, after)
    assert np.array_equal(after.cpu().numpy(), dr_ref.factors_all(14, 0, ep, 6, DR))
    for e in (whole, h0, h1):
        e.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched():
    def arm_asks(env):
        with pytest.raises(L.AmenvError):
            env.set_randomization(DR)
        with pytest.raises(L.AmenvError):
            env.dynamics_factors()

    H.check_refused(SW, lambda: _env("hexa_arm", "v2", 1, 64), arm_asks)
    with pytest.raises(L.AmenvError):
        _env("hexa_arm", "v2", 1, 64, n_joints=2, randomization=DR)
    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64, kernel="team"), DR)
    env = _env("quad", "v2", 1, 64, randomization=DR)
    env.reset()
    f0, i0 = env.get_state(); k0 = env.dynamics_factors().clone()
    bad = DR.to_c()
    bad.struct_size = 16
    assert env.lib.amenv_set_randomization(env._h, C.byref(bad)) == -1
    assert b"struct_size" in env.lib.amenv_last_error(env._h)
    for lo, hi in [(0.2, 1.0), (1.0, 4.5), (1.2, 1.1), (float("nan"), 1.0)]:
        r = DR.to_c()
        r.thrust_scale[0], r.thrust_scale[1] = lo, hi
        assert env.lib.amenv_set_randomization(env._h, C.byref(r)) == -1, (lo, hi)
    f1, i1 = env.get_state()
    assert torch.equal(f0, f1) and torch.equal(i0, i1) and torch.equal(env.dynamics_factors(), k0)   # the earlier ranges still hold
    env.set_randomization(None)
    assert torch.equal(env.dynamics_factors(), torch.ones_like(k0)) and "+dr" not in env.kernel_name
    env.close()


# ---- 8. PPO ---------------------------------------------------------------------------------------------------------------------
def test_ppo_fused_rollout_with_randomisation():
    n, T = 4096, 64
    env = amd.GpuWaypointEnv(n, vehicle="hexa", seed=2, max_episode_steps=60, randomization=DR)
    algo = PPO(env, fused_rollout=True, n_steps=T, n_epochs=2, batch_size=8192, seed=1)
    algo.learn(2 * T * n)
    assert len(algo.log) == 2 and all(math.isfinite(x) for rec in algo.log for x in rec.values())
    assert int(algo.buffer.dones.sum()) > 0
    env.close()
    venv = amd.GpuVecEnv(num_envs=256, vehicle="quad", task="v1_raw", randomization=DR)   # passed through **env_kwargs
    assert "+dr" in venv.backend.kernel_name and venv.backend.randomization is DR
    venv.backend.close()
    norm = ObsNormalizer(17)
    algo = PPO(amd.GpuWaypointEnv(n, task="v1_raw", seed=3, randomization=DR), obs_normalizer=norm, fused_rollout=True, n_steps=T,
               n_epochs=1, batch_size=8192, seed=1)
    algo.learn(2 * T * n)
    assert all(math.isfinite(x) for rec in algo.log for x in rec.values())
    norm.close()
