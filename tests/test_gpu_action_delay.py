"""Per-episode actuation latency of the rigid vehicles (amenv_set_action_delay) on the GPU: off is invisible; a
delayed handle given rows equals a plain twin given the APPLIED rows, which the test forms itself from tests/delay_ref.py (bit for bit, on
every step-kernel path); the published delay state is the reference's after every step; one fp32 case against the unchanged fp64 oracle;
one-launch rollouts and closed loops replay bit for bit through amenv_step, delay state included; restore, sharding, refusals, the
reference checkpoint at 10 and 40 ms, PPO."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import PPO, ActorCritic, evaluate_policy
from tests import delay_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, GID0 = 200, 1000                      # three full tiles + 8 ragged lanes; a non-zero env_id_offset
FULL = amd.ActionDelay(0, 8)
DR = amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1))
LAG = amd.RotorLag(0.015, 0.04)
NOISE = amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01)
ALL = dict(randomization=DR, rotor_lag=LAG, sensor_noise=NOISE)
HOVER = torch.tensor([1.0, 0.0, 0.0, 0.0])


def _env(vehicle="quad", task="v2", nwp=1, n=N, seed=4, **kw):
    kw.setdefault("max_episode_steps", 25)
    kw.setdefault("env_id_offset", GID0)
    return amd.GpuWaypointEnv(n, vehicle=vehicle, task=task, num_waypoints=nwp, seed=seed, **kw)


def _actions(T, n, seed, dev, wide=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if wide:   # near +-1 (and 0 / 2 on the collective): consecutive rows differ strongly
        a = torch.rand(T, n, 4, generator=g)
        a = torch.where(a < 0.5, -1.0 + 0.2 * a, 0.8 + 0.4 * a)
        a[..., 0] = torch.where(a[..., 0] < 0, 1.5 + a[..., 0], a[..., 0] + 0.7)
    else:
        a = torch.rand(T, n, 4, generator=g) * torch.tensor([0.6, 0.4, 0.4, 0.4]) + torch.tensor([0.7, -0.2, -0.2, -0.2])
    return a.to(dev).contiguous()


def _policy(od):
    torch.manual_seed(7)
    pol = ActorCritic(od, 4).cuda().flatten_()
    with torch.no_grad():
        pol.log_std.data.fill_(-1.2)
        pol.action_net.weight.mul_(30.0)
    return pol


def _buffers(T, n, od, dev):
    return dict(obs=torch.zeros(T + 1, n, od, device=dev), actions=torch.zeros(T, n, 4, device=dev), logp=torch.zeros(T, n, device=dev),
                values=torch.zeros(T, n, device=dev), rewards=torch.zeros(T, n, device=dev), dones=torch.zeros(T, n, dtype=torch.uint8, device=dev))


def _step_all(env, a):
    o, r, d, i = env.step(a)
    return [x.clone() for x in (o, r, d, i, env.terminal_obs, env.ep_return, env.ep_len)], d.bool()


def _same_step(ra, da, rb, db, t):
    for x, y in zip(ra[:4], rb[:4]):
        assert torch.equal(x, y), t
    for x, y in zip(ra[4:], rb[4:]):
        assert torch.equal(x[da], y[db]), t


def _same_state(a, b):
    fa, ia = a.get_state(); fb, ib = b.get_state()
    return torch.equal(fa, fb) and torch.equal(ia, ib)


def _history(env, z):
    """The test's own history of a handle whose delay was just turned on or that was just reset."""
    ep = env.get_state()[1][L.I_EPISODE].cpu().numpy()
    return delay_ref.History(env.cfg.seed, env.cfg.env_id_offset, ep, z.min_steps, z.max_steps)


def _push(hist, env, given, info):
    reset = (info.cpu().numpy().view(np.uint32) & delay_ref.WAS_RESET) != 0
    hist.push(given.cpu().numpy(), reset, env.get_state()[1][L.I_EPISODE].cpu().numpy())
    return reset


def _published(env):
    d, recent = env.action_delay_state()
    return d.cpu().numpy(), recent.cpu().numpy()


# ---- 1. off is invisible --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel", [("quad", "v2", 1, "auto"), ("hexa", "v2", 3, "lane"), ("quad", "v1_raw", 1, "helper")])
def test_delay_set_and_cleared_is_bit_invisible_step_and_rollout(vehicle, task, nwp, kernel):
    T = 40
    a = _env(vehicle, task, nwp, kernel=kernel)
    b = _env(vehicle, task, nwp, kernel=kernel)
    name = b.kernel_name
    b.set_action_delay(FULL)
    assert b.kernel_name == name + " +delay" and b.action_delay is FULL
    b.set_action_delay(None)
    assert b.kernel_name == name == a.kernel_name and b.action_delay is None
    assert torch.equal(a.reset(), b.reset())
    acts = _actions(T, N, 1, a.device)
    for t in range(T):
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, acts[t])
        _same_step(ra, da, rb, db, t)
    ra, rb = a.rollout(acts), b.rollout(acts)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert _same_state(a, b) and a.stats() == b.stats()
    a.close(); b.close()


def test_delay_set_and_cleared_is_bit_invisible_closed_loop():
    """The quadrotor at 4,096 envs is the lane-quad closed loop: after set + clear it is that form again."""
    n, T = 4096, 48
    a = _env(n=n)
    b = _env(n=n, action_delay=FULL)
    b.set_action_delay(None)
    assert a.kernel_name == b.kernel_name
    a.reset(); b.reset()
    od, dev = a.obs_dim, a.device
    pol = _policy(od)
    ba, bb = _buffers(T, n, od, dev), _buffers(T, n, od, dev)
    ia, ib = (torch.zeros(T, n, dtype=torch.int32, device=dev) for _ in range(2))
    a.rollout_policy(pol.flat_param, T, seed=9, draw0=3, info_bits=ia, **ba)
    b.rollout_policy(pol.flat_param, T, seed=9, draw0=3, info_bits=ib, **bb)
    torch.cuda.synchronize()
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
    assert torch.equal(ia, ib) and int(ba["dones"].sum()) > 0 and _same_state(a, b)
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
        assert _same_state(a, b), t
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
    a.reset(); b.reset()
    acts = _actions(T, N, 2, a.device, wide=True)
    ro = a.rollout(acts)
    for t in range(T):
        o, r, d, i = b.step(acts[t])
        assert torch.equal(ro["obs"][t], o) and torch.equal(ro["reward"][t], r) and torch.equal(ro["done"][t], d) and torch.equal(ro["info_bits"][t], i), t
    assert int(ro["done"].sum()) > N and _same_state(a, b) and a.stats() == b.stats()
    (da, ra), (db, rb) = a.action_delay_state(), b.action_delay_state()
    assert torch.equal(da, db) and torch.equal(ra, rb) and not torch.equal(ra, HOVER.to(ra.device).expand_as(ra))
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
    od, dev = env.obs_dim, env.device
    pol = _policy(od)
    env.reset(); ref.reset()
    warm = _actions(3, n, 8, dev, wide=True)
    for t in range(3):                                   # a start state with rows in the history
        env.step(warm[t])
    ref.set_action_delay(FULL)                           # (on -> on: keeps ref's own d and rows until the restore below)
    ref.set_state(*env.get_state())
    ref.set_action_delay_state(*env.action_delay_state())
    if "rotor_lag" in extra:
        ref.set_rotor_state(env.rotor_state())
    plain = hist = None
    if twin:
        plain = _env(vehicle, task, nwp, n=n, kernel="lane", **extra)
        plain.reset(); plain.set_state(*env.get_state())
        hist = _history(env, FULL)
        hist.d, hist.recent = (x.copy() for x in _published(env))
    kw = {}
    if norm:
        nrm = ObsNormalizer(od)
        nrm.update(env.observe())
        entry = ObsNormalizer(od); entry.set(*nrm.get())
        kw = dict(obs_normalizer=nrm)
    b = _buffers(T, n, od, dev)
    info = torch.zeros(T, n, dtype=torch.int32, device=dev); tobs = torch.full((T, n, od), float("nan"), device=dev)
    env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, info_bits=info, terminal_obs=tobs, **b, **kw)
    torch.cuda.synchronize()
    tr = (lambda x: entry.normalize(x)) if norm else (lambda x: x)
    lo, hi = pol.action_low, pol.action_high
    for t in range(T):
        given = torch.max(torch.min(b["actions"][t], hi), lo)
        o, r, d, i = ref.step(given)
        assert torch.equal(tr(o), b["obs"][t + 1]) and torch.equal(r, b["rewards"][t]) and torch.equal(d, b["dones"][t]) and torch.equal(i, info[t]), t
        dn = d.bool()
        if bool(dn.any()):
            assert torch.equal(tr(ref.terminal_obs[dn]), tobs[t][dn]), t
        if twin:
            _, rp, dp, _ = plain.step(torch.from_numpy(hist.applied(given.cpu().numpy())).to(dev))
            assert torch.equal(rp, b["rewards"][t]) and torch.equal(dp, b["dones"][t]), t
            _push(hist, ref, given, i)
    assert _same_state(env, ref) and env.stats()["episodes"] > 0
    (da, ra), (db, rb) = env.action_delay_state(), ref.action_delay_state()
    assert torch.equal(da, db) and torch.equal(ra, rb)
    if twin:
        assert np.array_equal(da.cpu().numpy(), hist.d) and np.array_equal(ra.cpu().numpy(), hist.recent)
    assert int(b["dones"].sum()) > 0
    env.close(); ref.close()
    if twin:
        plain.close()
    if norm:
        nrm.close(); entry.close()


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
    assert _same_state(a, b)
    (da_, ra_), (db_, rb_) = a.action_delay_state(), b.action_delay_state()
    assert torch.equal(da_, db_) and torch.equal(ra_, rb_)
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
    ow = whole.reset().clone(); o0 = h0.reset().clone(); o1 = h1.reset().clone()
    assert torch.equal(ow, torch.cat([o0, o1]))
    acts = _actions(T, n, 4, whole.device, wide=True)
    for t in range(T):
        ow, rw, dw, iw = (x.clone() for x in whole.step(acts[t]))
        p0 = [x.clone() for x in h0.step(acts[t, :cut])]
        p1 = [x.clone() for x in h1.step(acts[t, cut:])]
        for x, y, z in zip((ow, rw, dw, iw), p0, p1):
            assert torch.equal(x, torch.cat([y, z])), t
    for x, y, z in zip(whole.action_delay_state(), h0.action_delay_state(), h1.action_delay_state()):
        assert torch.equal(x, torch.cat([y, z]))
    for e in (whole, h0, h1):
        e.close()


# ---- 9. it changes how a policy flies -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8])
def test_reference_checkpoint_under_delay(d):
    """The reference checkpoint on the quadrotor, 1,024 episodes through evaluate_policy.  10 ms: success >= 88 % (the delayed oracle:
    92 of 95, 96.8 %; a sample of 95 has about 2 points of spread, the bar sits 9 points under).  40 ms: success < 10 %, crashes the
    majority of endings (the delayed oracle: 1 of 512, 511 crashed)."""
    env = amd.GpuWaypointEnv(1024, seed=99, action_delay=amd.ActionDelay(d))
    z = np.load(os.path.join(GOLD, "policy_2300000.npz"))
    pol = ActorCritic.from_sb3({k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("_")}, device=env.device)
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
def _octo_config(n):
    """A synthetic 8-rotor vehicle (the runtime-rotor-count kernels): rotors on a 0.3 m circle, alternating spin, pseudo-inverse allocation."""
    cfg = L.default_config("hexa", n)
    v = cfg.vehicle
    v.n_rotors, v.mass = 8, 3.0
    ang = np.arange(8) * np.pi / 4
    mix = np.stack([np.ones(8), 0.3 * np.sin(ang), -0.3 * np.cos(ang), 0.02 * (-1.0) ** np.arange(8)])
    alloc = np.linalg.pinv(mix)
    for r in range(8):
        for j in range(4):
            v.alloc[r * 4 + j] = alloc[r, j]
            v.mix[j * 8 + r] = mix[j, r]
        v.t_min[r], v.t_max[r] = 0.0, 2.0 * v.mass * v.g / 8
    cfg.env_id_offset = GID0
    return cfg


def test_delay_refusals_leave_everything_untouched():
    def refused(env, twin, call):
        env.reset(); twin.reset()
        with pytest.raises(L.AmenvError):
            call(env)
        assert "+delay" not in env.kernel_name and env.action_delay is None and env.kernel_name == env.lib.amenv_kernel_name(env._h).decode()
        a = _actions(1, env.num_envs, 3, env.device)[0]
        if env.act_dim != 4:
            a = torch.cat([a, torch.zeros(env.num_envs, env.act_dim - 4, device=env.device)], dim=1).contiguous()
        for x, y in zip(env.step(a), twin.step(a)):
            assert torch.equal(x, y)
        assert _same_state(env, twin)
        env.close(); twin.close()

    on = lambda e: e.set_action_delay(FULL)   # noqa: E731
    refused(_env("hexa_arm", n=64), _env("hexa_arm", n=64), on)
    with pytest.raises(L.AmenvError):
        _env("hexa_arm", n=64, n_joints=2, action_delay=FULL)
    refused(_env(n=64, dtype="f64"), _env(n=64, dtype="f64"), on)
    refused(_env(n=64, kernel="team"), _env(n=64, kernel="team"), on)
    refused(amd.GpuWaypointEnv(64, config=_octo_config(64)), amd.GpuWaypointEnv(64, config=_octo_config(64)), on)
    # bad struct_size / ranges through ctypes; the delay state while off
    env, twin = _env(n=64), _env(n=64)
    env.reset(); twin.reset()
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
    assert "+delay" not in env.kernel_name and env.kernel_name == env.lib.amenv_kernel_name(env._h).decode()
    a = _actions(1, 64, 3, env.device)[0]
    for x, y in zip(env.step(a), twin.step(a)):
        assert torch.equal(x, y)
    assert _same_state(env, twin)
    env.close(); twin.close()


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
