"""Body-rate actions with an inner rate loop (amenv_set_rate_control) on the GPU: the device function against the
numpy restatement; rate mode IS the unchanged step fed the equivalent moment rows, bit for bit, on every kernel that carries it (alone,
with randomisation -- the nominal inertia --, with rotor lag, behind the latency, beside the action history); the switch harness's
checks; the fp64 oracle fed the moment rows; the one-launch evaluation; the loop's closed form through amenv_step.

Shapes: 100 envs = one full 64-env tile and a partial one (padding lanes exist); max_episode_steps = 12 with T = 24 where episode ends must
occur; 40 envs for the evaluation form (16-env workgroups, the last one partial)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from tests import rate_ref
from tests import switch_harness as H
from tests.test_gpu_evaluate import check_against_twin

pytestmark = pytest.mark.gpu
SW = H.Switch("rate_control", "+rate", "set_rate_control", lambda e: ())

RATE = amd.RateControl()
NO_FF = amd.RateControl(max_rate=(4.0, 6.0, 2.0), gain=(30.0, 20.0, 8.0), gyro_feedforward=False)
WIDE = amd.DynamicsRandomization(mass=(0.6, 1.6), inertia=(0.5, 2.0), thrust=(0.8, 1.2))
LAG = amd.RotorLag(0.015, 0.04)
N, T, MES = 100, 24, 12
_env, _actions = H.make_env, H.actions


def _rate_env(vehicle, task, nwp, n=N, rate=RATE, **kw):
    kw.setdefault("max_episode_steps", MES)
    return _env(vehicle, task, nwp, n, rate_control=rate, **kw)


# ---- 1. the law -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,rate", [("quad", RATE), ("hexa", RATE), ("hexa", NO_FF), ("quad", NO_FF)])
def test_moment_actions_are_the_restated_law(vehicle, rate):
    """moment_actions (the kernels' own device function) against tests/rate_ref.py in fp64 on the constants as the device holds them:
    |delta a'_k| <= n_r * 2^-24 * S_k with n_r = 8, the roundings on the device function's longest path as written (w_cmd, the difference,
    u, the product and two fmas of the I u row, the sum with the feed-forward, the scaling by 1 / ms), S_k the sum of the absolute values
    of every term that enters a'_k.  Rates of +-8 rad/s lie beyond max_rate as well.  The thrust column comes back bit-equal."""
    env = _rate_env(vehicle, "v2", 1, rate=rate)
    check_the_law(env, rate, vehicle)
    env.close()


def check_the_law(env, rate, label):
    """The gate of the test above on a handle in rate mode (tests/test_gpu_generic_vehicles.py runs it on its vehicles)."""
    N = env.num_envs
    env.reset()
    g = torch.Generator().manual_seed(5)
    f, i = env.get_state()
    w = (torch.rand(3, N, generator=g) * 16.0 - 8.0)
    f[10:13] = w.to(f.device)
    env.set_state(f, i)
    rows = torch.rand(N, 4, generator=g) * torch.tensor([2.0, 2.4, 2.4, 2.4]) - torch.tensor([0.0, 1.2, 1.2, 1.2])
    got = env.moment_actions(rows.to(env.device)).cpu().numpy()
    want, S = rate_ref.moment_actions(rows.numpy(), w.numpy().T, *rate_ref.device_constants(env.cfg, rate.max_rate, rate.gain),
                                      gyro_feedforward=rate.gyro_feedforward)
    assert rate_ref.N_ROUNDINGS == 8
    assert np.array_equal(got[:, 0].view(np.uint32), rows.numpy()[:, 0].view(np.uint32))
    err = np.abs(got[:, 1:].astype(np.float64) - want[:, 1:])
    bound = rate_ref.N_ROUNDINGS * 2.0 ** -24 * S
    print(f"law {label} ff={rate.gyro_feedforward}: worst |delta a'| / (2^-24 S) = {(err / (2.0 ** -24 * S)).max():.2f} (bound {rate_ref.N_ROUNDINGS})")
    assert np.all(err <= bound), (err / bound).max()
    assert np.all(S > 0.0) and not np.array_equal(got[:, 1:], rows.numpy()[:, 1:])
    return float((err / (2.0 ** -24 * S)).max())


# ---- 2. the plumbing, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel,rate,extra,name", [
    ("quad", "v2", 1, "lane", RATE, {}, "step_kernel<"), ("hexa", "v2", 1, "helper", RATE, {}, "step_kernel_pw<float,NROT=6,KW=1,v2>"),
    ("hexa", "v2", 3, "helper", NO_FF, {}, "step_kernel_pw<float,NROT=6,KW=4,v2>"), ("quad", "v1_raw", 1, "helper", RATE, {}, "step_kernel_pw<float,NROT=4,KW=2,v1>"),
    ("hexa", "v2", 1, "helper", RATE, dict(randomization=WIDE), "step_kernel_pw<"), ("quad", "v2", 3, "lane", RATE, dict(randomization=WIDE), "step_kernel<"),
    ("hexa", "v2", 1, "lane", RATE, dict(rotor_lag=LAG), "step_kernel<"), ("quad", "v2", 1, "helper", NO_FF, dict(rotor_lag=LAG), "step_kernel_pw<")])
def test_rate_mode_is_the_step_fed_the_moment_rows(vehicle, task, nwp, kernel, rate, extra, name):
    """A is in rate mode; its twin B has rate control off, the same other switches, seed and state.  Every step A gets the command and B
    gets A.moment_actions(command) taken before the step: every output and the state agree bit for bit on every step, and the Monitor
    totals afterwards.  With a non-unit inertia range the twin shows that the loop uses the NOMINAL inertia (B's rows were formed with
    it, and B's dynamics divide by the episode's)."""
    a = _rate_env(vehicle, task, nwp, rate=rate, kernel=kernel, **extra)
    b = _env(vehicle, task, nwp, N, kernel=kernel, max_episode_steps=MES, **extra)
    assert a.kernel_name.startswith(name) and a.kernel_name.endswith(" +rate") and a.kernel_name == b.kernel_name + " +rate"
    assert torch.equal(a.reset(), b.reset())
    cmds = _actions(T, N, 3, a.device, wide=True, tipped=True)
    ended = 0
    for t in range(T):
        m = a.moment_actions(cmds[t])
        assert torch.equal(m[:, 0], cmds[t][:, 0])
        ra, da = H.step_all(a, cmds[t]); rb, db = H.step_all(b, m)
        H.same_step(ra, da, rb, db, t)
        H.same_state(a, b, t)
        ended += int(da.sum())
    assert ended >= N and a.stats() == b.stats()
    if "rotor_lag" in extra:
        assert torch.equal(a.rotor_state(), b.rotor_state())
    if "randomization" in extra:
        k_i = a.dynamics_factors()[:, 1]
        assert torch.equal(a.dynamics_factors(), b.dynamics_factors()) and float(k_i.max() - k_i.min()) > 0.5
    assert torch.equal(a.reset(), b.reset())
    a.close(); b.close()


# ---- 3. behind the latency, beside the history ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,nwp,kernel,hist", [("quad", 1, "helper", None), ("hexa", 3, "helper", None), ("hexa", 1, "lane", amd.ActionHistory(2)),
                                                     ("quad", 1, "helper", amd.ActionHistory(2))])
def test_the_rate_loop_runs_behind_the_latency(vehicle, nwp, kernel, hist):
    """A has ActionDelay(1, 3) and rate mode: the COMMAND is the delayed one, the rates are the current ones.  Its step must equal a plain
    handle C (no latency, no rate mode) stepped with moment_actions of the row A was given d steps ago, read from action_delay_state()
    before the step.  With ActionHistory(2) the appended rows are the given commands (what the delay's buffer holds after the push),
    never a'."""
    z = amd.ActionDelay(1, 3)
    a = _rate_env(vehicle, "v2", nwp, kernel=kernel, action_delay=z, action_history=hist)
    c = _env(vehicle, "v2", nwp, N, kernel=kernel, max_episode_steps=MES)
    assert a.kernel_name.endswith(" +delay +history 2 +rate" if hist else " +delay +rate")
    oa, oc = a.reset(), c.reset()
    assert torch.equal(oa[:, :c.obs_dim], oc)
    cmds = _actions(T, N, 8, a.device, wide=True)
    idx = torch.arange(N, device=a.device)
    ended = 0
    for t in range(T):
        d, recent = a.action_delay_state()
        assert int(d.min()) >= 1 and int(d.max()) <= 3
        applied = recent[idx, (d - 1).long()].contiguous()          # recent[:, k] was given k + 1 steps ago (hover where the episode is younger)
        m = a.moment_actions(applied)
        o, r, dn, info = (x.clone() for x in a.step(cmds[t]))
        o2, r2, dn2, info2 = c.step(m)
        assert torch.equal(o[:, :c.obs_dim], o2) and torch.equal(r, r2) and torch.equal(dn, dn2) and torch.equal(info, info2), t
        H.same_state(a, c, t)
        ended += int(dn.sum())
        if hist:
            _, after = a.action_delay_state()
            went_on = (info & L.INFO_WAS_RESET) == 0
            assert torch.equal(o[:, 20:24], after[:, 0]) and torch.equal(o[:, 24:28], after[:, 1]), t
            assert torch.equal(after[:, 0][went_on], cmds[t][went_on]), t
            hover = torch.tensor([1.0, 0.0, 0.0, 0.0], device=a.device)
            assert bool((o[:, 20:28][~went_on].reshape(-1, 4) == hover).all()), t
    assert ended >= N and a.stats() == c.stats()
    a.close(); c.close()


# ---- 4. the harness's checks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel", [("quad", "v2", 1, "auto"), ("hexa", "v2", 3, "helper"), ("hexa", "v1_raw", 1, "lane")])
def test_rate_set_and_cleared_is_bit_invisible_step_and_rollout(vehicle, task, nwp, kernel):
    a = _env(vehicle, task, nwp, N, kernel=kernel, max_episode_steps=MES)
    b = _env(vehicle, task, nwp, N, kernel=kernel, max_episode_steps=MES)
    H.check_set_and_cleared_step_and_rollout(SW, RATE, a, b, _actions(T, N, 1, a.device))
    a.close(); b.close()


@pytest.mark.parametrize("vehicle,task,nwp,n", [("quad", "v2", 1, 4096), ("hexa", "v2", 2, N)])
def test_rate_set_and_cleared_is_bit_invisible_closed_loop(vehicle, task, nwp, n):
    """The quadrotor at 4,096 envs is the lane-quad closed loop: after set + clear it is that form again."""
    a = _env(vehicle, task, nwp, n, max_episode_steps=MES)
    b = _rate_env(vehicle, task, nwp, n)
    H.check_set_and_cleared_closed_loop(SW, a, b, T)
    a.close(); b.close()


@pytest.mark.parametrize("vehicle,task,nwp,extra", [("quad", "v2", 1, {}), ("hexa", "v2", 3, dict(randomization=WIDE)), ("quad", "v1_raw", 1, dict(rotor_lag=LAG)),
                                                    ("hexa", "v2", 1, dict(action_delay=amd.ActionDelay(0, 3), action_history=amd.ActionHistory(1)))])
def test_rate_rollout_equals_steps(vehicle, task, nwp, extra):
    a = _rate_env(vehicle, task, nwp, **extra)
    b = _rate_env(vehicle, task, nwp, **extra)
    H.check_rollout_equals_steps(a, b, _actions(T, N, 2, a.device, wide=True), min_ended=N - 1, side=())
    a.close(); b.close()


@pytest.mark.parametrize("vehicle,task,nwp,n,norm,extra", [("quad", "v2", 1, N, False, {}), ("hexa", "v1_raw", 1, N, True, {}), ("quad", "v2", 1, 4096, True, dict(randomization=WIDE)),
                                                           ("hexa", "v2", 2, N, False, dict(rotor_lag=LAG, action_delay=amd.ActionDelay(0, 2)))])
def test_rate_closed_loop_replays_bit_for_bit(vehicle, task, nwp, n, norm, extra):
    """The closed loop samples COMMANDS; replaying the recorded clipped commands through amenv_step on a rate-mode lane-kernel handle
    reproduces every row.  (quad, v2, one waypoint at 4,096 envs: a config the lane-quad closed loop would serve runs the one-lane form.)"""
    env = _rate_env(vehicle, task, nwp, n, **extra)
    ref = _rate_env(vehicle, task, nwp, n, kernel="lane", **extra)
    H.check_closed_loop_replays(env, ref, T, norm=norm, side=()).close()


def test_rate_two_shards_equal_one_handle():
    cut = 36
    whole = _rate_env("hexa", "v2", 1, seed=13)
    h0 = _rate_env("hexa", "v2", 1, cut, seed=13)
    h1 = _rate_env("hexa", "v2", 1, N - cut, seed=13, env_id_offset=cut)
    H.check_two_shards(whole, h0, h1, cut, _actions(T, N, 4, whole.device, wide=True), side=())
    for e in (whole, h0, h1):
        e.close()


def _raw(env, max_rate=RATE.max_rate, gain=RATE.gain):
    c = L.RateControlC()
    for k in range(3):
        c.max_rate[k], c.gain[k] = max_rate[k], gain[k]
    c.gyro_feedforward = 1
    return env.lib.amenv_set_rate_control(env._h, C.byref(c))


def test_rate_refusals_leave_everything_untouched():
    def asks(env):
        with pytest.raises(L.AmenvError):
            env.set_rate_control(RATE)
        with pytest.raises(L.AmenvError, match="off"):
            env.moment_actions(torch.zeros(env.num_envs, env.act_dim))

    H.check_refused(SW, lambda: _env("hexa_arm", "v2", 1, 64), asks)
    with pytest.raises(L.AmenvError):
        _env("hexa_arm", "v2", 1, 64, n_joints=2, rate_control=RATE)
    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64, dtype="f64"), RATE, "fp32")
    H.check_refused(SW, lambda: amd.GpuWaypointEnv(64, config=H.octo_config(64)), RATE, "4 or 6 rotors")
    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64, kernel="team"), RATE, "lane-quad")
    H.check_refused(SW, lambda: _env("hexa", "v2", 1, 64), amd.RateControl(gain=(25.0, 250.0, 10.0)), "gain")     # gain * dt = 1.25

    def bad_values(env):      # through ctypes: the C ABI's own checks
        inf, nan = float("inf"), float("nan")
        for k in range(3):
            for bad in (0.0, -1.0, inf, nan, 1e300):
                mr = list(RATE.max_rate); mr[k] = bad
                assert _raw(env, max_rate=mr) == -1 and b"max_rate" in env.lib.amenv_last_error(env._h), (k, bad)
            for bad in (0.0, -25.0, inf, nan, 200.0, 1e-300):
                g = list(RATE.gain); g[k] = bad
                assert _raw(env, gain=g) == -1 and b"gain" in env.lib.amenv_last_error(env._h), (k, bad)
        assert env.lib.amenv_rate_moment_actions(env._h, None, None, None) == -1
        with pytest.raises(L.AmenvError, match="off"):
            env.moment_actions(torch.zeros(64, 4))

    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64), bad_values)
    env = _env("quad", "v2", 1, 64)        # a refusal on a handle where it is on keeps the old values; the baseline refuses a rate-mode env
    env.set_rate_control(NO_FF)
    assert _raw(env, gain=(0.0, 1.0, 1.0)) == -1 and env.kernel_name.endswith(" +rate") and env.rate_control is NO_FF
    with pytest.raises(L.AmenvError, match="rate"):
        amd.PidWaypointPolicy.for_env(env)
    env.set_rate_control(None)
    amd.PidWaypointPolicy.for_env(env)
    env.close()


def test_ppo_fused_rollout_with_rate_control():
    H.check_ppo_fused_rollout_replays(SW, 4096, 16, rate_control=RATE)


# ---- 5. the oracle gate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel", [("quad", "v2", 1, "auto"), ("hexa", "v2", 3, "lane"), ("hexa", "v2", 1, "helper"), ("quad", "v1_raw", 1, "helper")])
def test_rate_mode_matches_the_oracle_fed_the_moment_rows(vehicle, task, nwp, kernel):
    """Teacher-forced per step: the unchanged fp64 oracle starts from the GPU's state and is fed moment_actions(command); its state after the
    step is the GPU's to the fp32 tolerance of tests/test_gpu_rotor_lag.py::test_lagged_kernels_match_the_pinned_oracle, 1e-5 relative
    to max(1, |x|).  The one-launch rollout of a twin publishes the same observation rows to the same tolerance."""
    env = _rate_env(vehicle, task, nwp, seed=8, kernel=kernel)
    twin = _rate_env(vehicle, task, nwp, seed=8, kernel=kernel)
    check_against_the_oracle_fed_the_moment_rows(env, twin, f"{vehicle} {task} {nwp} {kernel}")
    env.close(); twin.close()


def check_against_the_oracle_fed_the_moment_rows(env, twin, label, T=T):
    """The gate of the test above on two handles in rate mode with the same seed (tests/test_gpu_generic_vehicles.py runs it on its vehicles)."""
    tol = 1e-5
    N = env.num_envs
    env.reset(); twin.reset()
    cmds = _actions(T, N, 6, env.device, wide=True)
    ro = twin.rollout(cmds)["obs"].cpu().numpy().astype(np.float64)
    orc = O.OracleEnv(H.oracle_cfg(env))
    worst, worst_o, ended, compared = 0.0, 0.0, 0, 0
    for t in range(T):
        f_prev, i_prev = (x.cpu().numpy() for x in env.get_state())
        m = env.moment_actions(cmds[t]).cpu().numpy()
        env.step(cmds[t])
        f_new = env.get_state()[0].cpu().numpy().astype(np.float64)
        done = env.done.cpu().numpy() != 0
        orc.fstate[:] = f_prev.astype(np.float64); orc.istate[:] = i_prev
        out = orc.step(m)
        on = ~done & (out["done"] == 0)
        ended += int(done.sum()); compared += int(on.sum())
        if not on.any():          # (the step in which every env runs into the time limit)
            continue
        err = np.abs(orc.fstate[:13][:, on] - f_new[:13][:, on]) / np.maximum(1.0, np.abs(orc.fstate[:13][:, on]))
        worst = max(worst, float(err.max()))
        oo = out["obs"][on].astype(np.float64)
        worst_o = max(worst_o, float((np.abs(ro[t][on] - oo) / np.maximum(1.0, np.abs(oo))).max()))
    print(f"rate gate {label}: state {worst:.3e} rollout rows {worst_o:.3e} (tol {tol:g}), {ended} episode ends")
    assert worst <= tol, worst
    assert worst_o <= tol, worst_o
    assert ended > 0 and compared > T * N // 2
    return worst, worst_o


# ---- 6. the one-launch evaluation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,nwp,deterministic,extra", [("quad", 1, True, {}), ("hexa", 2, False, {}), ("hexa", 1, True, dict(randomization=WIDE, rotor_lag=LAG))])
def test_fused_evaluation_in_rate_mode_is_the_twin_rollout_reduced(vehicle, nwp, deterministic, extra):
    """tests/test_gpu_evaluate.py's method on 40 envs (16-env workgroups, the last one partial), 2 episodes each: counts identical, returns bit-equal."""
    n, mes = 40, 30
    env = _rate_env(vehicle, "v2", nwp, n, max_episode_steps=mes, **extra)
    twin = _rate_env(vehicle, "v2", nwp, n, max_episode_steps=mes, block_size=64, **extra)
    _, c, steps, _ = check_against_twin(env, twin, lambda: H.policy(env.obs_dim), per_env=2, max_steps=2 * (mes + 2), deterministic=deterministic)
    assert bool((c[:, 0] == 2).all()) and steps <= 2 * (mes + 1)
    env.close(); twin.close()


# ---- 7. physical sanity on the device --------------------------------------------------------------------------------------------------
def test_rate_loop_closed_form_on_the_device():
    """tests/test_rate_control_cpu.py's closed form through amenv_step: the reference quadrotor (diagonal inertia) from rest, thrust action 1,
    a constant single-axis rate command, 100 steps: w_n = w_cmd (1 - (1 - gain dt)^n).  Gate: the CPU gate 1e-6 |w_cmd| widened by the fp32
    per-step parity bound, 1e-5 relative to max(1, |w|)."""
    n = 96
    env = _rate_env("quad", "v2", 1, n, max_episode_steps=1000, auto_reset=False)
    env.reset()
    dt = float(env.cfg.task.dt)
    w_cmd = np.array([1.0, -0.8, 1.0])
    axis = np.arange(n) % 3
    cmd = torch.zeros(n, 4)
    cmd[:, 0] = 1.0
    for i in range(n):
        cmd[i, 1 + axis[i]] = float(w_cmd[axis[i]] / RATE.max_rate[axis[i]])
    cmd = cmd.to(env.device)
    gain = np.array(RATE.gain)[axis]
    worst = 0.0
    for k in range(1, 101):
        _, _, done, _ = env.step(cmd)
        assert int(done.sum()) == 0, k
        w = env.get_state()[0][10:13].cpu().numpy().astype(np.float64)
        got = w[axis, np.arange(n)]
        want = rate_ref.closed_form_rate(w_cmd[axis], gain, dt, k)
        gate = 1e-6 * np.abs(w_cmd[axis]) + 1e-5 * np.maximum(1.0, np.abs(want))
        worst = max(worst, float((np.abs(got - want) / gate).max()))
        assert np.all(np.abs(got - want) <= gate), k
        off = w.copy(); off[axis, np.arange(n)] = 0.0
        assert np.abs(off).max() <= 1e-4, k          # (Ixz = 1e-2 Ixx: what the held feed-forward misses inside a step, ~1e-5 rad/s)
    print(f"closed form on the device: worst error / gate = {worst:.3f}")
    env.close()
