"""Per-episode actuation latency of the rigid vehicles (amenv_set_action_delay) on the GPU: off is invisible; a
delayed handle given rows equals a plain twin given the APPLIED rows, which the test forms itself from tests/delay_ref.py (bit for bit, on
every step-kernel path); the published delay state is the reference's after every step; one fp32 case against the unchanged fp64 oracle;
one-launch rollouts and closed loops replay bit for bit through amenv_step, delay state included; restore, sharding, refusals, the
reference checkpoint at 10 and 40 ms, PPO."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.ppo import PPO, evaluate_policy
from tests import delay_ref
from tests import switch_harness as H

pytestmark = pytest.mark.gpu
SW = H.ACTION_DELAY

N, GID0 = 200, 1000                      # three full tiles + 8 ragged lanes; a non-zero env_id_offset
FULL = amd.ActionDelay(0, 8)
DR = amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1))
LAG = amd.RotorLag(0.015, 0.04)
NOISE = amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01)
ALL = dict(randomization=DR, rotor_lag=LAG, sensor_noise=NOISE)
HOVER = torch.tensor([1.0, 0.0, 0.0, 0.0])


def _env(vehicle="quad", task="v2", nwp=1, n=N, seed=4, **kw):
    kw.setdefault("env_id_offset", GID0)
    return H.make_env(vehicle, task, nwp, n, seed, **kw)


_actions, _step_all, _same_step, _same_state = H.actions, H.step_all, H.same_step, H.same_state
_history, _push = H.delay_history, H.push_history


def _published(env):
    d, recent = env.action_delay_state()
    return d.cpu().numpy(), recent.cpu().numpy()


# ---- 1. off is invisible --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel", [("quad", "v2", 1, "auto"), ("hexa", "v2", 3, "lane"), ("quad", "v1_raw", 1, "helper")])
def test_delay_set_and_cleared_is_bit_invisible_step_and_rollout(vehicle, task, nwp, kernel):
    T = 40
    a = _env(vehicle, task, nwp, kernel=kernel)
    b = _env(vehicle, task, nwp, kernel=kernel)
    H.check_set_and_cleared_step_and_rollout(SW, FULL, a, b, _actions(T, N, 1, a.device))
    a.close(); b.close()


def test_delay_set_and_cleared_is_bit_invisible_closed_loop():
    """The quadrotor at 4,096 envs is the lane-quad closed loop: after set + clear it is that form again."""
    n, T = 4096, 48
    a = _env(n=n)
    b = _env(n=n, action_delay=FULL)
    H.check_set_and_cleared_closed_loop(SW, a, b, T)
    a.close(); b.close()


# ---- 2. the gate: twin replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel,kw,z,extra", [
    ("quad", "v2", 1, "auto", {}, FULL, {}),                          # step_kernel_pw, 256-thread form
    ("hexa", "v2", 3, "helper", {}, FULL, {}),                        # step_kernel_pw, 128-thread form
    ("quad", "v1_raw", 1, "auto", {}, FULL, {}),
    ("hexa", "v2", 1, "lane", dict(block_size=64), FULL, {}),         # step_kernel
    ("quad", "v2", 1, "auto", {}, amd.ActionDelay(0), {}),            # d = 0 everywhere: the given rows themselves
    ("hexa", "v2", 2, "auto", {}, FULL, ALL),                         # with randomisation + lag + noise on both handles
    ("quad", "v2", 1, "lane", {}, amd.ActionDelay(3, 8), dict(rotor_lag=LAG))])
def test_delayed_handle_equals_a_plain_twin_given_the_applied_rows(vehicle, task, nwp, kernel, kw, z, extra):
    """The twin never hears of the delay: the test takes d from delay_ref and the rows from its own history (hover refill on reset)."""
    T = 80
    a = _env(vehicle, task, nwp, kernel=kernel, action_delay=z, **kw, **extra)
    b = _env(vehicle, task, nwp, kernel=kernel, **kw, **extra)
    assert a.kernel_name == b.kernel_name + " +delay"
    assert torch.equal(a.reset(), b.reset())
    hist = _history(a, z)
    acts = _actions(T, N, 11, a.device, wide=True)
    ended = differed = 0
    for t in range(T):
        applied = torch.from_numpy(hist.applied(acts[t].cpu().numpy())).to(a.device)
        differed += int((applied != acts[t]).any(dim=1).sum())
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, applied)
        _same_step(ra, da, rb, db, t)
        _same_state(a, b, t)
        ended += int(_push(hist, a, acts[t], ra[3]).sum())
    assert a.stats() == b.stats() and ended > N
    assert differed == 0 if z.max_steps == 0 else differed > T * N // 2
    if "rotor_lag" in extra:
        assert torch.equal(a.rotor_state(), b.rotor_state())
    a.close(); b.close()


# ---- 3. published state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,nwp,kernel", [("quad", 1, "auto"), ("hexa", 3, "helper"), ("hexa", 1, "lane")])
def test_published_delay_state_follows_the_reference(vehicle, nwp, kernel):
    T = 60
    env = _env(vehicle, "v2", nwp, kernel=kernel, max_episode_steps=12)
    env.reset()
    env.set_action_delay(FULL)                     # off -> on: every env draws for its CURRENT episode, hover rows
    hist = _history(env, FULL)
    d, recent = _published(env)
    assert d.dtype == np.int32 and recent.shape == (N, 8, 4)
    assert np.array_equal(d, hist.d) and np.array_equal(recent, hist.recent) and len(set(d.tolist())) == 9
    env.reset()                                    # amenv_reset: the next episode number
    hist = _history(env, FULL)
    d, recent = _published(env)
    assert np.array_equal(d, hist.d) and np.array_equal(recent, hist.recent)
    acts = _actions(T, N, 5, env.device, wide=True)
    changed = 0
    for t in range(T):
        d_prev = hist.d.copy()
        env.step(acts[t])
        reset = _push(hist, env, acts[t], env.info_bits)
        d, recent = _published(env)
        assert np.array_equal(d, hist.d), t
        assert np.array_equal(recent.view(np.uint32), hist.recent.view(np.uint32)), t
        assert np.array_equal(d[~reset], d_prev[~reset]), t            # d changes at episode starts only
        changed += int((d != d_prev).sum())
    assert changed > N // 2
    # a new range keeps every env's d and rows; amenv_reset(mask) redraws (from the new range) and refills the masked envs only
    env.set_action_delay(amd.ActionDelay(7, 8))
    d1, r1 = _published(env)
    assert np.array_equal(d1, d) and np.array_equal(r1, recent)
    mask = torch.zeros(N, dtype=torch.uint8); mask[::3] = 1
    env.reset(mask)
    m = mask.numpy() != 0
    ep = env.get_state()[1][L.I_EPISODE].cpu().numpy()
    d2, r2 = _published(env)
    assert np.array_equal(d2[m], delay_ref.draw_all(env.cfg.seed, GID0, ep, 7, 8)[m]) and np.all(d2[m] >= 7)
    assert np.array_equal(r2[m], np.tile(delay_ref.HOVER, (int(m.sum()), 8, 1)))
    assert np.array_equal(d2[~m], d1[~m]) and np.array_equal(r2[~m], r1[~m]) and not np.array_equal(r2[~m], np.tile(delay_ref.HOVER, (int((~m).sum()), 8, 1)))
    env.close()


# ---- 4. independent of the twin: the unchanged fp64 oracle ------------------------------------------------------------------------
def test_delayed_kernel_matches_the_delayed_oracle():
    """fp32 quadrotor against delay_ref.DelayedOracle, teacher-forced per step (the oracle is re-seated on the GPU state; its history is
    its own).  State within 1e-5 max(1, |x|), observation likewise; flag bits equal except threshold flips, counted as
    test_gpu_parity.test_closed_loop_teacher_forced_with_resets counts them (3 in 614,400 env-steps there; 16,000 here: at most 1)."""
    T = 80
    env = _env(action_delay=FULL, seed=5)
    orc = delay_ref.DelayedOracle(O.reference_quad_config(num_envs=N, seed=5), 0, 8)
    orc.cfg.task.max_episode_steps = 25
    orc.cfg.env_id_offset = GID0
    env.reset(); orc.reset()
    assert np.array_equal(_published(env)[0], orc.hist.d)
    acts = _actions(T, N, 21, env.device, wide=True)
    acts[..., 1:] *= 0.05
    worst = worst_o = 0.0
    flips = dones = 0
    for t in range(T):
        f, i = env.get_state()
        orc.env.fstate[:] = f.cpu().numpy().astype(np.float64); orc.env.istate[:] = i.cpu().numpy()
        obs, rew, done, info = env.step(acts[t])
        o = orc.step(acts[t].cpu().numpy())
        f, i = (x.cpu().numpy() for x in env.get_state())
        gi = info.cpu().numpy().view(np.uint32)
        bad = (gi & 127) != (o["info"] & 127)
        flips += int(bad.sum())
        ok = ~bad
        nd = ok & (o["done"] == 0)
        dn = ok & (o["done"] != 0)
        dones += int(dn.sum())
        assert np.array_equal(done.cpu().numpy()[ok], o["done"][ok]) and np.array_equal(i[:, ok], orc.env.istate[:, ok]), t
        assert np.array_equal(f[:, dn].astype(np.float64), orc.env.fstate[:, dn]), t          # reset states are bit-exact
        if nd.any():      # (envs that survive their 25 steps are truncated in the same step: no env is left then)
            err = np.abs(f[:13][:, nd] - orc.env.fstate[:13][:, nd]) / np.maximum(1.0, np.abs(orc.env.fstate[:13][:, nd]))
            worst = max(worst, float(err.max()))
        eo = np.abs(obs.cpu().numpy()[ok].astype(np.float64) - o["obs"][ok]) / np.maximum(1.0, np.abs(o["obs"][ok]))
        worst_o = max(worst_o, float(eo.max()))
        d, recent = _published(env)
        assert np.array_equal(d[ok], orc.hist.d[ok]) and np.array_equal(recent[ok], orc.hist.recent[ok]), t
        for j in np.flatnonzero(bad):     # a flipped env: the oracle's history follows the GPU's episode
            orc.hist.d[j] = d[j]; orc.hist.recent[j] = recent[j]
    print(f"delay vs oracle: state {worst:.3e} obs {worst_o:.3e} flips {flips} episode ends {dones}")
    assert worst <= 1e-5 and worst_o <= 1e-5, (worst, worst_o)
    assert flips <= 1 and dones > N
    env.close()


# ---- 5. amenv_rollout = steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,extra", [("quad", "v2", 1, {}), ("hexa", "v2", 3, ALL), ("quad", "v1_raw", 1, {})])
def test_delayed_rollout_equals_steps(vehicle, task, nwp, extra):
    T = 64
    a = _env(vehicle, task, nwp, action_delay=FULL, **extra)
    b = _env(vehicle, task, nwp, action_delay=FULL, **extra)
    H.check_rollout_equals_steps(a, b, _actions(T, N, 2, a.device, wide=True), min_ended=N, side=(SW,))
    ra = a.action_delay_state()[1]
    assert not torch.equal(ra, HOVER.to(ra.device).expand_as(ra))
    a.close(); b.close()


# ---- 6. the closed loop replays through amenv_step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,n,norm,extra,twin", [
    ("quad", "v2", 1, 300, False, {}, True),            # 16-env workgroups; a config the lane-quad closed loop would serve
    ("hexa", "v2", 2, 12000, False, {}, False),         # 64-env workgroups
    ("hexa", "v2", 1, 40000, False, {}, False),         # 128-env workgroups
    ("quad", "v1_raw", 1, 300, True, {}, False),        # NORM
    ("quad", "v2", 1, 300, True, ALL, False)])
def test_delayed_closed_loop_replays_bit_for_bit(vehicle, task, nwp, n, norm, extra, twin):
    T = 64
    env = _env(vehicle, task, nwp, n=n, action_delay=FULL, **extra)
    ref = _env(vehicle, task, nwp, n=n, kernel="lane", action_delay=amd.ActionDelay(1), **extra)
    assert env.kernel_name.endswith(" +delay")
    dev = env.device
    plain = hist = None

    def start(env, ref):
        nonlocal plain, hist
        warm = _actions(3, n, 8, dev, wide=True)
        for t in range(3):                               # a start state with rows in the history
            env.step(warm[t])
        ref.set_action_delay(FULL)                       # (on -> on: keeps ref's own d and rows until the restore below)
        ref.set_state(*env.get_state())
        ref.set_action_delay_state(*env.action_delay_state())
        if "rotor_lag" in extra:
            ref.set_rotor_state(env.rotor_state())
        if twin:
            plain = _env(vehicle, task, nwp, n=n, kernel="lane", **extra)
            plain.reset(); plain.set_state(*env.get_state())
            hist = _history(env, FULL)
            hist.d, hist.recent = (x.copy() for x in _published(env))

    def plain_twin(t, given, o, r, d, i):
        _, rp, dp, _ = plain.step(torch.from_numpy(hist.applied(given.cpu().numpy())).to(dev))
        assert torch.equal(rp, r) and torch.equal(dp, d), t
        _push(hist, ref, given, i)

    run = H.check_closed_loop_replays(env, ref, T, norm=norm, side=(SW,), prepare=start, each_step=plain_twin if twin else None, totals=False)
    assert env.stats()["episodes"] > 0
    if twin:
        da, ra = _published(env)
        assert np.array_equal(da, hist.d) and np.array_equal(ra, hist.recent)
        plain.close()
    run.close()


# ---- 7. without auto-reset ----------------------------------------------------------------------------------------------------------
def test_without_auto_reset_a_finished_env_keeps_d_and_its_history():
    env = _env(auto_reset=False, max_episode_steps=5, action_delay=FULL)
    env.reset()
    hist = _history(env, FULL)
    acts = _actions(12, N, 6, env.device)
    for t in range(12):
        env.step(acts[t])
        hist.push(acts[t].cpu().numpy())                 # no episode starts: rows keep entering, nothing is redrawn or refilled
        d, recent = _published(env)
        assert np.array_equal(d, hist.d) and np.array_equal(recent, hist.recent), t
    assert bool(env.done.bool().all()) and not (env.info_bits.cpu().numpy() & delay_ref.WAS_RESET).any()
    env.close()


# ---- 8. restore and sharding ------------------------------------------------------------------------------------------------------
def test_restore_into_a_fresh_handle_and_set_state_alone():
    a = _env("hexa", "v2", 2, seed=5, action_delay=FULL, randomization=DR)
    a.reset()
    acts = _actions(50, N, 9, a.device, wide=True)
    for t in range(30):
        a.step(acts[t])
    f, i = a.get_state()
    d, recent = a.action_delay_state()
    b = _env("hexa", "v2", 2, seed=5, randomization=DR)
    b.reset()
    b.set_action_delay(FULL)
    d0, r0 = b.action_delay_state()
    b.set_state(f, i)                                    # set_state alone leaves the delay state as it was, whatever the step field says
    d1, r1 = b.action_delay_state()
    assert torch.equal(d0, d1) and torch.equal(r0, r1) and not torch.equal(r1, recent)
    b.set_action_delay_state(d, recent)
    d2, r2 = b.action_delay_state()
    assert torch.equal(d2, d) and torch.equal(r2, recent)
    for t in range(30, 50):
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, acts[t])
        _same_step(ra, da, rb, db, t)
    _same_state(a, b)
    SW.same_side_state(a, b)
    # the setter clamps d to 0..8
    b.set_action_delay_state(torch.full((N,), 99, dtype=torch.int32), recent)
    assert bool((b.action_delay_state()[0] == 8).all())
    b.set_action_delay_state(torch.full((N,), -3, dtype=torch.int32), recent)
    assert bool((b.action_delay_state()[0] == 0).all())
    a.close(); b.close()


def test_two_shards_equal_one_handle():
    n, T, cut = 200, 60, 72                              # a cut that is no multiple of the tile
    whole = _env("hexa", "v2", 1, n=n, seed=13, max_episode_steps=20, action_delay=FULL)
    h0 = _env("hexa", "v2", 1, n=cut, seed=13, max_episode_steps=20, action_delay=FULL)
    h1 = _env("hexa", "v2", 1, n=n - cut, seed=13, max_episode_steps=20, action_delay=FULL, env_id_offset=GID0 + cut)
    H.check_two_shards(whole, h0, h1, cut, _actions(T, n, 4, whole.device, wide=True), side=(SW,))
    for e in (whole, h0, h1):
        e.close()


# ---- 9. it changes how a policy flies -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8])
def test_reference_checkpoint_under_delay(d):
    """The reference checkpoint on the quadrotor, 1,024 episodes through evaluate_policy.  10 ms: success >= 88 % (the delayed oracle:
    92 of 95, 96.8 %; a sample of 95 has about 2 points of spread, the bar sits 9 points under).  40 ms: success < 10 %, crashes the
    majority of endings (the delayed oracle: 1 of 512, 511 crashed)."""
    env = amd.GpuWaypointEnv(1024, seed=99, action_delay=amd.ActionDelay(d))
    pol = H.fixture_policy(env.device)
    env.reset()
    env.stats(reset=True)
    evaluate_policy(pol, env, n_eval_episodes=1024)
    s = env.stats()
    print(f"delay {d}: {s['episodes']} episodes, {s['success']} success, {s['crashed']} crashed")
    assert s["episodes"] >= 1024
    if d == 2:
        assert s["success"] >= 0.88 * s["episodes"], s
    else:
        assert s["success"] < 0.10 * s["episodes"] and s["crashed"] > 0.5 * s["episodes"], s
    env.close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------
def test_delay_refusals_leave_everything_untouched():
    H.check_refused(SW, lambda: _env("hexa_arm", n=64), FULL)
    with pytest.raises(L.AmenvError):
        _env("hexa_arm", n=64, n_joints=2, action_delay=FULL)
    H.check_refused(SW, lambda: _env(n=64, dtype="f64"), FULL)
    H.check_refused(SW, lambda: _env(n=64, kernel="team"), FULL)
    H.check_refused(SW, lambda: amd.GpuWaypointEnv(64, config=H.octo_config(64, GID0)), FULL)

    def bad_struct_and_off(env):     # bad struct_size / ranges through ctypes; the delay state while off
        bad = FULL._as_c()
        bad.struct_size = 8
        assert env.lib.amenv_set_action_delay(env._h, C.byref(bad)) == -1 and b"struct_size" in env.lib.amenv_last_error(env._h)
        for lo, hi in [(3, 2), (0, 9), (-1, 4)]:
            c = FULL._as_c()
            c.min_steps, c.max_steps = lo, hi
            assert env.lib.amenv_set_action_delay(env._h, C.byref(c)) == -1, (lo, hi)
        with pytest.raises(L.AmenvError, match="off"):
            env.action_delay_state()
        with pytest.raises(L.AmenvError, match="off"):
            env.set_action_delay_state(torch.zeros(64, dtype=torch.int32), torch.zeros(64, 8, 4))

    H.check_refused(SW, lambda: _env(n=64), bad_struct_and_off)


# ---- 11. PPO ----------------------------------------------------------------------------------------------------------------------
def test_ppo_fused_rollout_with_action_delay():
    n, T = 4096, 16
    env = amd.GpuWaypointEnv(n, seed=2, max_episode_steps=12, action_delay=amd.ActionDelay(0, 4))
    assert env.kernel_name.endswith(" +delay")
    algo = PPO(env, fused_rollout=True, n_steps=T, n_epochs=2, batch_size=8192, seed=1)
    algo.learn(3 * T * n)
    assert len(algo.log) == 3 and all(math.isfinite(x) for rec in algo.log for x in rec.values())
    assert all(rec["episodes"] > 0 for rec in algo.log) and int(algo.buffer.dones.sum()) > 0     # (PPO reads and clears the Monitor totals every iteration)
    d, recent = env.action_delay_state()
    assert int(d.min()) >= 0 and int(d.max()) <= 4 and len(set(d.cpu().tolist())) == 5
    env.close()
    vec = amd.GpuVecEnv(num_envs=64, action_delay=amd.ActionDelay(1))     # the kwarg reaches the env through the VecEnv
    assert vec.backend.kernel_name.endswith(" +delay")
    vec.close()
