"""Sensor noise on the rigid vehicles' observations (amenv_set_sensor_noise) on the GPU: off is invisible; the samples
are the numpy restatement's, bit for bit; the true dynamics, rewards and Monitor totals do not move; every row a kernel forms -- step,
terminal, post-reset, reset(), observe() -- is the UNCHANGED fp64 oracle's observation of the perturbed state (tests/noise_ref.py); the
one-launch rollout and the closed loop replay bit for bit through amenv_step and the policy reads the noisy rows; shards; refusals; PPO."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from tests import noise_ref
from tests import switch_harness as H
from tests.test_rollout_v1_cpu import RunningMeanStd

pytestmark = pytest.mark.gpu
SW = H.SENSOR_NOISE

N = 200       # three full 64-env tiles + 8 ragged lanes
Z = amd.SensorNoise(position=0.03, velocity=0.08, rate=0.05, attitude=0.02)
Z_NO_ATT = amd.SensorNoise(position=0.05, velocity=0.02, rate=0.1, attitude=0.0)
Z_BIG = amd.SensorNoise(position=0.3, velocity=0.5, rate=0.4, attitude=0.2)     # the closed-loop cases: the policy must visibly read it
LAG = amd.RotorLag(0.015, 0.04)
WIDE = amd.DynamicsRandomization(mass=(0.6, 1.6), inertia=(0.5, 2.0), thrust=(0.8, 1.2))
OBS_TOL = 1e-5   # the project's fp32 observation gate, relative to max(1, |x|)


def _env(vehicle, task, nwp, n=N, seed=4, **kw):
    return H.make_env(vehicle, task, nwp, n, seed, **kw)


_actions = functools.partial(H.actions, tipped=True)     # a third of the envs is pushed over hard: crashes and out-of-bounds ends join the truncations
_step_all, _ocfg = H.step_all, H.oracle_cfg


def _state(env):
    f, i = env.get_state()
    return f.cpu().numpy().astype(np.float64), i.cpu().numpy()


def _expected(env, z, f=None, i=None):
    if f is None:
        f, i = _state(env)
    return noise_ref.expected_obs(_ocfg(env), f, i, z.sigmas, int(env.cfg.seed), int(env.cfg.env_id_offset))


def _obs_err(got, want):
    got, want = got.cpu().numpy().astype(np.float64), want.astype(np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ---- 1. off is invisible --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,nwp,kernel,kname", [("quad", 1, "auto", "step_kernel_pw<float,NROT=4,KW=1,v2>"), ("hexa", 3, "lane", "step_kernel<float,NROT=6,KW=4,v2>")])
def test_set_then_cleared_and_zero_sigmas_are_bit_invisible(vehicle, nwp, kernel, kname):
    """Against a twin that never heard of the noise: a handle that had it on and cleared it, and a handle given all-zero sigmas."""
    T = 40
    twin = _env(vehicle, "v2", nwp, kernel=kernel)
    cleared = _env(vehicle, "v2", nwp, kernel=kernel, sensor_noise=Z)
    assert cleared.kernel_name == twin.kernel_name + " +noise" and cleared.sensor_noise is Z and kname in twin.kernel_name
    cleared.set_sensor_noise(None)
    zero = _env(vehicle, "v2", nwp, kernel=kernel, sensor_noise=amd.SensorNoise())
    acts = _actions(T, N, 1, twin.device)
    pol = H.policy(twin.obs_dim)
    for other in (cleared, zero):
        a = _env(vehicle, "v2", nwp, kernel=kernel) if other is zero else twin
        assert other.kernel_name == a.kernel_name and "+noise" not in other.kernel_name
        assert torch.equal(a.reset(), other.reset())
        H.check_same_steps_and_rollout(a, other, acts)
        assert torch.equal(a.observe(), other.observe())
        H.check_same_closed_loop(a, other, pol, 16, info_bits=False, ends=False)
        # (the merged statistics agree to rounding, with the tolerances of tests/test_gpu_rollout_v1.py::test_normaliser_inside_the_launch)
        (ma, va, ca), (mb, vb, cb) = H.check_same_closed_loop(a, other, pol, 16, norm=True, info_bits=False, ends=False)
        assert ca == cb
        np.testing.assert_allclose(mb, ma, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(vb, va, rtol=1e-10, atol=1e-14 * float(np.max(ma ** 2 + va)))
        H.same_state(a, other)
        assert a.stats() == other.stats()
        if a is not twin:
            a.close()
    twin.close(); cleared.close(); zero.close()


# ---- 2. the samples are the restatement's -----------------------------------------------------------------------------------------
def test_samples_match_the_restatement_after_every_step():
    T, seed, gid0 = 40, 21, 100000
    env = _env("quad", "v2", 1, seed=seed, env_id_offset=gid0, max_episode_steps=12, sensor_noise=Z)
    env.reset()

    def check():
        s = env.sensor_noise_samples().cpu().numpy()
        _, i = _state(env)
        assert s.shape == (N, 12) and s.dtype == np.float32
        assert np.array_equal(s, noise_ref.samples_all(seed, gid0, i[L.I_EPISODE], i[L.I_STEP])), "samples differ from the restatement"
        return s, i

    prev, i0 = check()
    acts = _actions(T, N, 3, env.device)
    for t in range(T):
        env.step(acts[t])
        s, i = check()
        assert int((s != prev).any(1).sum()) == N, t      # every env's samples move with every step
        prev = s
    assert int(i[L.I_EPISODE].min()) > int(i0[L.I_EPISODE].max())       # every env went through resets
    env.set_sensor_noise(None)                                            # the samples do not depend on the switch
    assert np.array_equal(env.sensor_noise_samples().cpu().numpy(), prev)
    env.close()


# ---- 3. the true dynamics are untouched -------------------------------------------------------------------------------------------
def test_noise_leaves_state_reward_and_totals_alone():
    T = 300
    noisy = _env("hexa", "v2", 1, seed=6, sensor_noise=Z)
    clean = _env("hexa", "v2", 1, seed=6)
    on, oc = noisy.reset().clone(), clean.reset().clone()
    assert not torch.equal(on, oc)
    acts = _actions(8, N, 5, noisy.device)
    differ = 0
    for t in range(T):
        rn, dn = _step_all(noisy, acts[t % 8]); rc, dc = _step_all(clean, acts[t % 8])
        for x, y in zip(rn[1:4], rc[1:4]):                 # reward, done, info
            assert torch.equal(x, y), t
        for x, y in zip(rn[5:], rc[5:]):                   # Monitor's return / length of the envs that ended
            assert torch.equal(x[dn], y[dc]), t
        differ += int((rn[0] != rc[0]).any(1).sum())
        if bool(dn.any()):
            assert not torch.equal(rn[4][dn], rc[4][dc]), t
        fn, i_n = noisy.get_state(); fc, ic = clean.get_state()
        assert torch.equal(fn, fc) and torch.equal(i_n, ic), t
    assert differ == T * N and noisy.stats() == clean.stats() and noisy.stats()["episodes"] > N
    noisy.close(); clean.close()


# ---- 4. the gate: every row against the oracle's observation of the perturbed state -----------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kw,z,kname", [
    ("quad", "v2", 1, dict(kernel="auto", env_id_offset=7777), Z, "step_kernel_pw<float,NROT=4,KW=1,v2>"),          # observation-wave path
    ("hexa", "v2", 3, dict(kernel="auto", randomization=WIDE, rotor_lag=LAG), Z, "step_kernel_pw<float,NROT=6,KW=4,v2>"),   # 128-thread helper form
    ("quad", "v1_raw", 1, dict(kernel="auto"), Z_NO_ATT, "step_kernel_pw<float,NROT=4,KW=2,v1>"),
    ("quad", "v1_scaled", 1, dict(kernel="lane"), Z, "step_kernel<float,NROT=4,KW=2,v1>"),
    ("hexa", "v2", 1, dict(block_size=128), Z, "step_kernel<float,NROT=6,KW=1,v2> block=128")])
def test_rows_match_the_oracle_on_the_perturbed_state(vehicle, task, nwp, kw, z, kname):
    """Step and post-reset rows from get_state() after the step; terminal rows through an auto_reset=False twin that is set to the
    handle's state before every step (its rows against its own get_state(), the handle's terminal rows bit-equal to them)."""
    T = 60
    env = _env(vehicle, task, nwp, seed=8, sensor_noise=z, **kw)
    twin = _env(vehicle, task, nwp, seed=8, sensor_noise=z, auto_reset=False, **kw)
    assert kname in env.kernel_name and env.kernel_name.endswith(" +noise") and twin.kernel_name == env.kernel_name
    lag = kw.get("rotor_lag") is not None
    o0 = env.reset().clone()
    worst = _obs_err(o0, _expected(env, z))
    assert worst <= OBS_TOL, ("reset row", worst)
    acts = _actions(T, N, 6, env.device)
    ended = resets = 0
    for t in range(T):
        f_prev, i_prev = env.get_state()
        twin.set_state(f_prev, i_prev)
        if lag:
            twin.set_rotor_state(env.rotor_state())
        (o, r, d, info, tobs, _, _), dn = _step_all(env, acts[t])
        (ot, rt, dt, _, _, _, _), dnt = _step_all(twin, acts[t])
        assert torch.equal(d, dt) and torch.equal(r, rt), t
        err = _obs_err(o, _expected(env, z))                       # step rows and post-reset rows
        err_t = _obs_err(ot, _expected(twin, z))                   # step rows and terminal rows
        print(f"t={t} step/post-reset row error {err:.3e} twin (terminal) row error {err_t:.3e} ended {int(dn.sum())}")
        worst = max(worst, err, err_t)
        assert err <= OBS_TOL and err_t <= OBS_TOL, (t, err, err_t)
        assert torch.equal(o[~dn], ot[~dn]), t
        if bool(dn.any()):
            assert torch.equal(tobs[dn], ot[dn]), t              # the terminal row the handle published
            assert not torch.equal(o[dn], ot[dn]), t
            ended += int(dn.sum())
            resets += int(((info & L.INFO_WAS_RESET) != 0).sum())
    assert ended > N and resets == ended
    last = env.obs.clone()
    a, b = env.observe(), env.observe()
    assert torch.equal(a, b) and torch.equal(a, last)              # idempotent, and the row the last step returned
    assert _obs_err(a, _expected(env, z)) <= OBS_TOL
    clean = noise_ref.expected_obs(_ocfg(env), *_state(env), (0.0, 0.0, 0.0, 0.0), 8, int(env.cfg.env_id_offset))
    assert _obs_err(a, clean) > 100 * OBS_TOL                      # (the gate would see a row without noise)
    if z.attitude == 0.0:                                          # a zero sigma leaves its components numerically the clean ones
        assert np.abs(a.cpu().numpy()[:, 6:10].astype(np.float64) - clean[:, 6:10]).max() <= OBS_TOL
    print("worst row error", worst)
    env.close(); twin.close()


# ---- 5. amenv_rollout equals steps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["v2", "v1_raw"])
def test_noisy_rollout_equals_steps(task):
    T = 64
    a = _env("quad", task, 1, sensor_noise=Z)
    b = _env("quad", task, 1, sensor_noise=Z)
    ro = H.check_rollout_equals_steps(a, b, _actions(T, N, 2, a.device), min_ended=N)
    assert torch.equal(a.observe(), ro["obs"][T - 1])
    a.close(); b.close()


# ---- 6. closed loop -----------------------------------------------------------------------------------------------------------------
# sizes: 300 runs the 16-env workgroups, 12000 the 64-env ones, 40000 the 128-env ones (as tests/test_gpu_rollout_v1.py)
# the last case is one of the six forms that keep 12-20 B of scratch per lane
@pytest.mark.parametrize("vehicle,task,nwp,n,norm,extra", [("quad", "v2", 1, 300, False, {}), ("quad", "v1_raw", 1, 12000, True, {}),
                                                           ("hexa", "v2", 2, 40000, False, dict(randomization=WIDE, rotor_lag=LAG)),
                                                           ("hexa", "v2", 3, 12000, True, dict(rotor_lag=LAG))])
def test_noisy_closed_loop_replays_and_the_policy_reads_the_noisy_rows(vehicle, task, nwp, n, norm, extra):
    """quad / v2 / one waypoint is a config the lane-quad closed loop serves: with the noise on it runs the one-lane-per-env form."""
    T = 32
    env = _env(vehicle, task, nwp, n=n, sensor_noise=Z_BIG, **extra)
    ref = _env(vehicle, task, nwp, n=n, kernel="lane", sensor_noise=Z_BIG, **extra)
    clean = _env(vehicle, task, nwp, n=n, kernel="lane", **extra)
    assert "step_kernel<" in ref.kernel_name and ref.kernel_name.endswith("+noise")
    od = env.obs_dim
    c_rows = [clean.reset().clone()]
    raw_rows = []

    def clean_twin(t, act, o, r, d, i):
        raw_rows.append(o.clone())
        oc, rc, dc, _ = clean.step(act)
        assert torch.equal(rc, r) and torch.equal(dc, d), t       # the clean twin flies the same true trajectory
        c_rows.append(oc.clone())

    run = H.check_closed_loop_replays(env, ref, T, norm=norm, side=(H.ROTOR_LAG,) if extra else (), each_step=clean_twin)
    b, pol, tr = run.b, run.pol, run.tr
    H.same_state(env, clean)
    if norm:   # the `update` sums counted the noisy raw rows 1..T (tolerances: tests/test_gpu_rollout_v1.py::test_normaliser_inside_the_launch)
        mean0, var0, count0 = run.entry.get()
        mean1, var1, count1 = run.nrm.get()
        rms = RunningMeanStd(od)
        rms.mean, rms.var, rms.count = mean0.copy(), var0.copy(), count0
        for row in raw_rows:
            rms.update(row.cpu().numpy().astype(np.float64))
        assert count1 == count0 + T * n
        np.testing.assert_allclose(mean1, rms.mean, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(var1, rms.var, rtol=1e-10, atol=1e-14 * float(np.max(rms.mean ** 2 + rms.var)))

    def values_of(rows):
        with torch.no_grad():
            return pol.value_net(pol.mlp_extractor.value_net(rows.reshape(T * n, od))).reshape(-1)

    v32 = values_of(b["obs"][:T])
    v_clean = values_of(tr(torch.stack(c_rows[:T])))
    bound = 3e-2 * max(1.0, float(v32.abs().max()))
    d_noisy, d_clean = float((b["values"].reshape(-1) - v32).abs().max()), float((b["values"].reshape(-1) - v_clean).abs().max())
    print(f"values: against the recorded (noisy) rows {d_noisy:.3e}, against the clean twin's rows {d_clean:.3e}, bound {bound:.3e}")
    assert d_noisy < bound
    assert d_clean > bound
    run.close(); clean.close()


# ---- 7. shards ------------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_one_handle():
    T, cut = 40, 128
    whole = _env("hexa", "v2", 1, seed=13, max_episode_steps=20, sensor_noise=Z)
    h0 = _env("hexa", "v2", 1, n=cut, seed=13, max_episode_steps=20, sensor_noise=Z)
    h1 = _env("hexa", "v2", 1, n=N - cut, seed=13, max_episode_steps=20, sensor_noise=Z, env_id_offset=cut)
    H.check_two_shards(whole, h0, h1, cut, _actions(T, N, 4, whole.device), side=(SW,))
    assert whole.stats()["episodes"] >= N        # 40 steps of 20-step episodes: every env ended once
    for e in (whole, h0, h1):
        e.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def _unit_row(env):
    return torch.rand(env.num_envs, env.act_dim, generator=torch.Generator().manual_seed(3)).to(env.device)


_refused = functools.partial(H.check_refused, SW, action=_unit_row)


def test_refusals_leave_the_handle_untouched():
    _refused(lambda: _env("hexa_arm", "v2", 1, n=64), Z, "rigid")
    _refused(lambda: amd.GpuWaypointEnv(64, config=H.octo_config(64)), Z, "4 or 6 rotors")
    _refused(lambda: _env("quad", "v2", 1, n=64, dtype="f64"), Z, "fp32")
    _refused(lambda: _env("quad", "v2", 1, n=64, kernel="team"), Z, "lane-quad")
    _refused(lambda: _env("quad", "v2", 1, n=64, max_episode_steps=2 ** 22 - 1), Z, "max_episode_steps")
    with pytest.raises(L.AmenvError):
        _env("hexa_arm", "v2", 1, n=64, n_joints=2, sensor_noise=Z)

    def bad_struct(env):
        c = Z.to_c()
        c.struct_size = 16
        assert env.lib.amenv_set_sensor_noise(env._h, C.byref(c)) == -1 and b"struct_size" in env.lib.amenv_last_error(env._h)

    def bad_sigmas(env):
        for k, name in enumerate(("sigma_position", "sigma_velocity", "sigma_rate", "sigma_attitude")):
            for bad in (-0.01, 1.5, float("nan"), float("inf"), -float("inf")):
                c = Z.to_c()
                setattr(c, name, bad)
                assert env.lib.amenv_set_sensor_noise(env._h, C.byref(c)) == -1, (name, bad)
                assert name.encode() in env.lib.amenv_last_error(env._h)
        assert env.lib.amenv_sensor_noise_samples(env._h, None, None) == -1

    _refused(lambda: _env("quad", "v2", 1, n=64), bad_struct)
    _refused(lambda: _env("hexa", "v2", 2, n=64), bad_sigmas)
    # the bound itself is served
    ok = _env("quad", "v2", 1, n=64, max_episode_steps=2 ** 22 - 2, sensor_noise=Z)
    assert ok.kernel_name.endswith("+noise")
    ok.close()


# ---- 9. PPO -----------------------------------------------------------------------------------------------------------------------------
def test_ppo_fused_rollout_with_sensor_noise():
    n, T = 4096, 16
    H.check_ppo_fused_rollout_replays(SW, n, T, sensor_noise=Z)      # the policy was trained on the noisy rows
