"""Per-episode rotor failure (amenv_set_rotor_failure) on the GPU: a failure that never happens or leaves the rotor
whole changes no output bit; plan and multipliers are the numpy restatement's (tests/fail_ref.py), change with the episode and flip at the
onset; the kernels match the UNCHANGED fp64 oracle given each env's scaled mixer column; a dead rotor pulls the way its mixer column says;
the switch harness's checks alone and beside rotor lag + latency + sensor noise; the one-launch evaluation; refusals and re-keying.

Shapes: 100 envs = one full 64-env tile and a partial one (padding lanes exist); max_episode_steps = 12 with T = 24..30, so that episodes
pass their onset (3..9) and restart; 40 envs for the evaluation form (16-env workgroups, the last one partial)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from tests import dr_ref, fail_ref
from tests import switch_harness as H
from tests.test_gpu_evaluate import check_against_twin

pytestmark = pytest.mark.gpu
SW = H.Switch("rotor_failure", "+fail", "set_rotor_failure", lambda e: tuple(e.rotor_failure_state()))

FAIL = amd.RotorFailure(probability=1.0, onset=(3, 9), remaining=(0.0, 0.5))
SOME = amd.RotorFailure(probability=0.5, onset=(3, 9), remaining=(0.0, 0.5))
NEVER = amd.RotorFailure(probability=0.0, onset=(3, 9), remaining=(0.0, 0.5))
WHOLE = amd.RotorFailure(probability=1.0, onset=(3, 9), remaining=(1.0, 1.0))
ONE = amd.DynamicsRandomization()
WIDE = amd.DynamicsRandomization(mass=(0.6, 1.6), inertia=(0.5, 2.0), thrust=(0.8, 1.2))
LDS = dict(rotor_lag=amd.RotorLag(0.015, 0.04), action_delay=amd.ActionDelay(0, 3), sensor_noise=amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01))
CONFIGS = [("quad", "v2", 1), ("hexa", "v2", 3), ("quad", "v1_raw", 1)]
N, T, MES = 100, 24, 12
_actions = H.actions


def _env(vehicle, task, nwp, n=N, **kw):
    kw.setdefault("max_episode_steps", MES)
    return H.make_env(vehicle, task, nwp, n, **kw)


def _fail_env(vehicle, task, nwp, n=N, fail=FAIL, **kw):
    return _env(vehicle, task, nwp, n, rotor_failure=fail, **kw)


# ---- 1. a failure that changes nothing changes no bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fail", [NEVER, WHOLE], ids=["never", "whole"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("vehicle,task,nwp", CONFIGS)
@pytest.mark.parametrize("kernel", ["auto", "lane"])
def test_no_effective_failure_is_bit_identical(vehicle, task, nwp, dtype, kernel, fail):
    """probability 0, and probability 1 with remaining (1, 1): every output of step, rollout and (fp32) the closed loop with and without the
    normaliser equals a handle with DynamicsRandomization() only."""
    a = _env(vehicle, task, nwp, dtype=dtype, kernel=kernel, randomization=ONE)
    b = _fail_env(vehicle, task, nwp, dtype=dtype, kernel=kernel, randomization=ONE, fail=fail)
    assert b.kernel_name == a.kernel_name + " +fail" and a.kernel_name.endswith(" +dr")
    assert torch.equal(a.reset(), b.reset())
    plan, fac = b.rotor_failure_state()
    assert torch.equal(fac, torch.ones(N, b.n_rotors, device=b.device)) and bool(((plan[:, 0] >= 0) == (fail is WHOLE)).all())
    H.check_same_steps_and_rollout(a, b, _actions(T, N, 1, a.device, wide=True))
    if dtype == "f32":
        a.reset(); b.reset()
        pol = H.policy(a.obs_dim)
        H.check_same_closed_loop(a, b, pol, T)
        (ma, va, ca), (mb, vb, cb) = H.check_same_closed_loop(a, b, pol, T, norm=True)
        assert ca == cb
        np.testing.assert_allclose(ma, mb, rtol=1e-10, atol=1e-12); np.testing.assert_allclose(va, vb, rtol=1e-10, atol=1e-12)
        H.same_state(a, b)
    a.close(); b.close()


# ---- 2. plan and multipliers are the restatement's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,dtype,rotors", [("quad", "f32", None), ("hexa", "f64", [0, 2, 3, 5])])
def test_plan_matches_restatement_and_follows_episodes(vehicle, dtype, rotors):
    """Bit for bit after the reset and after every one of 300 steps, on 512 envs with 40-step episodes: the plan is the restatement's of the
    env's current (gid, episode) -- so it stays while the episode counter does and is the new episode's when that moves --, the multipliers
    are 1 until the stored step reaches the onset and f on the failed rotor from then on, and dynamics_factors() stays the episode's."""
    n, T, seed = 512, 300, 21
    p = amd.RotorFailure(probability=0.8, onset=(2, 30), remaining=(0.1, 0.6), rotors=rotors)
    dr = amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1))
    env = _env(vehicle, "v2", 1, n, seed=seed, dtype=dtype, max_episode_steps=40, randomization=dr, rotor_failure=p)
    env.reset()
    nr = env.n_rotors
    cache = {}

    def restated(ep):
        rows = [cache.setdefault((i, int(e)), fail_ref.plan(seed, i, int(e), nr, p)) for i, e in enumerate(ep)]
        return np.array([[r, o] for r, o, _ in rows], np.int32), np.array([f for _, _, f in rows], np.float32)

    def read():
        plan, fac = (x.cpu().numpy() for x in env.rotor_failure_state())
        ist = env.get_state()[1].cpu().numpy()
        return plan, fac, ist[L.I_STEP], ist[L.I_EPISODE], env.dynamics_factors().cpu().numpy()

    acts = _actions(T, n, 5, env.device)
    prev = None
    changed = moved = flipped = 0
    for t in range(T + 1):
        plan, fac, step, ep, drf = read()
        want_plan, want_f = restated(ep)
        assert plan.dtype == np.int32 and fac.dtype == np.float32 and plan.shape == (n, 2) and fac.shape == (n, nr)
        assert np.array_equal(plan, want_plan), t
        assert np.array_equal(fac.view(np.uint32), fail_ref.effective_all(want_plan, want_f, step, nr).view(np.uint32)), t
        if prev is not None:
            same = ep == prev[3]
            assert np.array_equal(plan[same], prev[0][same]) and np.array_equal(drf[same], prev[4][same]), t     # constant within an episode
            changed += int((~same).sum()); moved += int(np.any(plan[~same] != prev[0][~same], axis=1).sum())
            on = same & (plan[:, 0] >= 0)
            at = on & (step == plan[:, 1]) & (prev[2] == plan[:, 1] - 1)                                        # the stored step has just reached the onset
            idx = np.nonzero(at)[0]
            assert np.array_equal(prev[1][idx], np.ones((len(idx), nr), np.float32)), t                          # 1 up to here ...
            assert np.array_equal(fac[idx, plan[idx, 0]], want_f[idx]) and np.all((fac[idx] != 1.0).sum(axis=1) <= 1), t        # ... f from here on
            flipped += len(idx)
        prev = (plan, fac, step, ep, drf)
        if t < T:
            env.step(acts[t])
    failing = np.array([r for r, _, _ in cache.values()])
    assert changed > n and moved > 0.8 * changed and flipped > n
    assert 0.7 < (failing >= 0).mean() < 0.9                                    # probability 0.8
    assert set(failing[failing >= 0]) == set(rotors or range(nr))             # every admissible rotor, and no other
    env.close()


# ---- 3. the kernels against the per-env oracle -------------------------------------------------------------------------------------------
def check_against_per_env_oracle(env, dtype, T, min_share):
    """tests/test_gpu_randomization.py::check_against_per_env_oracle with the failed rotor's column scaled: env i's oracle is the unchanged
    fp64 oracle on fail_ref.oracle_config(cfg, factors of env i's episode, multipliers read before the step).  fp64 <= 1e-12, fp32 <= 1e-5
    relative to max(1, |x|); reset states bit for bit.  At least min_share of the (env, step) pairs ran before their env's onset and at
    least min_share from it on."""
    n = env.num_envs
    env.reset()
    base = H.oracle_cfg(env)
    acts = _actions(T, n, 6, env.device, wide=True)
    tol = 1e-12 if dtype == "f64" else 1e-5
    worst, ended, before, after = 0.0, 0, 0, 0
    for t in range(T):
        f_prev, i_prev = (x.cpu().numpy() for x in env.get_state())
        fac = env.dynamics_factors().cpu().numpy()
        plan, ff = (x.cpu().numpy() for x in env.rotor_failure_state())
        hit = (plan[:, 0] >= 0) & (i_prev[L.I_STEP] >= plan[:, 1])
        assert np.all(ff[~hit] == 1.0) and np.all((ff[hit] != 1.0).sum(axis=1) == 1), t               # (remaining <= 0.5: a hit shows)
        before += int(((plan[:, 0] >= 0) & ~hit).sum()); after += int(hit.sum())
        env.step(acts[t])
        f_new, i_new = (x.cpu().numpy().astype(np.float64) for x in env.get_state())
        done = env.done.cpu().numpy()
        a = acts[t].cpu().numpy()
        for i in range(n):
            orc = O.OracleEnv(fail_ref.oracle_config(base, fac[i], ff[i], gid=i, dtype=dtype))
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
    print(f"rotor-failure gate {env.kernel_name}: state {worst:.3e} (tol {tol:g}), {ended} episode ends, {before} / {after} of {n * T} (env, step) pairs before / from the onset")
    assert worst <= tol, worst
    assert ended > 0
    assert before >= min_share * n * T and after >= min_share * n * T, (before, after)
    return worst


@pytest.mark.parametrize("vehicle,task,nwp,dtype,kernel", [("quad", "v2", 1, "f64", "lane"), ("quad", "v2", 1, "f64", "helper"),
                                                           ("hexa", "v2", 3, "f64", "lane"), ("hexa", "v2", 3, "f64", "helper"),
                                                           ("quad", "v1_raw", 1, "f64", "lane"), ("quad", "v1_raw", 1, "f64", "helper"),
                                                           ("quad", "v2", 1, "f32", "auto"), ("hexa", "v2", 3, "f32", "lane"),
                                                           ("quad", "v2", 1, "f32", "lane"), ("hexa", "v2", 3, "f32", "auto")])
def test_kernels_match_the_oracle_with_a_failed_rotor(vehicle, task, nwp, dtype, kernel):
    """Every episode fails: probability 1, onset (3, 9), remaining (0, 0.5), beside the wide randomisation ranges; actions near +-1 saturate
    rotors.  With 13-call episodes about 46 % of the pairs lie before the onset (tests/test_rotor_failure_cpu.py); at least 25 % must, and
    25 % behind it."""
    env = _fail_env(vehicle, task, nwp, 64, seed=8, dtype=dtype, kernel=kernel, randomization=WIDE)
    check_against_per_env_oracle(env, dtype, 30, 0.25)
    env.close()


def test_kernels_match_the_oracle_with_half_the_episodes_failing():
    env = _fail_env("hexa", "v2", 3, 64, seed=8, dtype="f64", kernel="lane", randomization=WIDE, fail=SOME)
    check_against_per_env_oracle(env, "f64", 30, 0.15)     # (half of the ~46 % / 54 % the restatement gives, less the binomial spread of 64 x 3 episodes: 192 episodes, sigma 3.6 % of them)
    ep_plans = env.rotor_failure_state()[0][:, 0].cpu().numpy()
    assert 0 < (ep_plans >= 0).sum() < 64
    env.close()


# ---- 4. it does something ------------------------------------------------------------------------------------------------------------
def test_a_dead_rotor_pulls_the_way_its_mixer_column_says():
    """Hexacopter, fp64, rotor 2 dead from step 0, the hover action from the reset state, one step: the vehicle sinks against its
    failure-free twin, and each body rate moves against the sign of the rotor's entry in the mixer's moment rows (diagonal inertia)."""
    dead = amd.RotorFailure(probability=1.0, onset=(0, 0), remaining=(0.0, 0.0), rotors=[2])
    a = _env("hexa", "v2", 1, 64, dtype="f64", randomization=ONE)
    b = _fail_env("hexa", "v2", 1, 64, dtype="f64", randomization=ONE, fail=dead)
    assert torch.equal(a.reset(), b.reset())
    plan, fac = b.rotor_failure_state()
    assert bool((plan == torch.tensor([2, 0], dtype=torch.int32, device=b.device)).all())
    assert torch.equal(fac, torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 1.0], device=b.device).expand(64, 6))
    hover = torch.tensor([1.0, 0.0, 0.0, 0.0], device=a.device).expand(64, 4).contiguous()
    a.step(hover); b.step(hover)
    fa, fb = a.get_state()[0], b.get_state()[0]
    assert bool((fb[5] < fa[5]).all())                                       # vz
    mix = np.array(a.cfg.vehicle.mix[:24]).reshape(4, 6)
    checked = 0
    for k in range(3):
        if mix[1 + k, 2] != 0.0:
            dw = (fb[10 + k] - fa[10 + k]).cpu().numpy()
            assert np.all(np.sign(dw) == -np.sign(mix[1 + k, 2])), k
            checked += 1
    assert checked == 3
    a.close(); b.close()


# ---- 5. the harness's checks, alone and beside rotor lag + latency + sensor noise ---------------------------------------------------------
EXTRAS = [pytest.param({}, id="alone"), pytest.param(LDS, id="lag+delay+noise")]


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("vehicle,task,nwp,kernel", [("quad", "v2", 1, "auto"), ("hexa", "v2", 3, "helper"), ("hexa", "v1_raw", 1, "lane")])
def test_fail_set_and_cleared_is_bit_invisible_step_and_rollout(vehicle, task, nwp, kernel, extra):
    a = _env(vehicle, task, nwp, kernel=kernel, **extra)
    b = _env(vehicle, task, nwp, kernel=kernel, **extra)
    H.check_set_and_cleared_step_and_rollout(SW, FAIL, a, b, _actions(T, N, 1, a.device))
    a.close(); b.close()


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("vehicle,task,nwp,n", [("quad", "v2", 1, 4096), ("hexa", "v2", 2, N)])
def test_fail_set_and_cleared_is_bit_invisible_closed_loop(vehicle, task, nwp, n, extra):
    """The quadrotor at 4,096 envs is the lane-quad closed loop: after set + clear it is that form again."""
    a = _env(vehicle, task, nwp, n, **extra)
    b = _fail_env(vehicle, task, nwp, n, **extra)
    H.check_set_and_cleared_closed_loop(SW, a, b, T)
    a.close(); b.close()


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("vehicle,task,nwp,dtype", [("quad", "v2", 1, "f32"), ("hexa", "v2", 3, "f32"), ("quad", "v1_raw", 1, "f32"), ("hexa", "v2", 1, "f64")])
def test_fail_rollout_equals_steps(vehicle, task, nwp, dtype, extra):
    if dtype == "f64":
        extra = {k: v for k, v in extra.items() if k == "rotor_lag"}      # (noise and latency are fp32 only)
    a = _fail_env(vehicle, task, nwp, dtype=dtype, randomization=WIDE, **extra)
    b = _fail_env(vehicle, task, nwp, dtype=dtype, randomization=WIDE, **extra)
    H.check_rollout_equals_steps(a, b, _actions(T, N, 2, a.device, wide=True), min_ended=N - 1, side=(SW, H.RANDOMIZATION))
    a.close(); b.close()


def test_rollout_entered_in_the_middle_of_an_episode():
    """After 7 steps most envs are past their onset (3..9) and the others about to reach it: a rollout launched there equals steps from
    there (the entry compares the loaded step with >=), and set_state of that state into a fresh handle gives the same."""
    a, b, c = (_fail_env("hexa", "v2", 1, randomization=WIDE) for _ in range(3))
    acts = _actions(T, N, 2, a.device, wide=True)
    assert torch.equal(a.reset(), b.reset())
    c.reset()
    for t in range(7):
        a.step(acts[t]); b.step(acts[t])
    plan, fac = a.rotor_failure_state()
    past = (fac != 1.0).any(dim=1)
    assert 0.3 * N < int(past.sum()) < N
    c.set_state(*a.get_state())
    H.same_tensors(SW.side_state(a), SW.side_state(c))
    ro, rc = a.rollout(acts[7:]), c.rollout(acts[7:])
    for t in range(7, T):
        o, r, d, i = b.step(acts[t])
        for got in (ro, rc):
            assert torch.equal(got["obs"][t - 7], o) and torch.equal(got["reward"][t - 7], r) and torch.equal(got["done"][t - 7], d), t
    H.same_state(a, b); H.same_state(c, b)
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("vehicle,task,nwp,n", [("quad", "v2", 1, 300), ("hexa", "v2", 2, 4096), ("quad", "v1_raw", 1, 12000), ("hexa", "v1_scaled", 1, 40000)])
def test_fail_closed_loop_replays_bit_for_bit(vehicle, task, nwp, n, norm, extra):
    """16-, 64- and 128-env workgroups; with the normaliser and the extras the factors live in LDS.  (quad, v2, one waypoint: a config the
    lane-quad closed loop would serve runs the one-lane form while the failure is set.)"""
    env = _fail_env(vehicle, task, nwp, n, randomization=WIDE, **extra)
    ref = _fail_env(vehicle, task, nwp, n, kernel="lane", randomization=WIDE, **extra)
    assert env.kernel_name.endswith(" +fail")
    H.check_closed_loop_replays(env, ref, T, norm=norm, side=(SW, H.RANDOMIZATION)).close()


@pytest.mark.parametrize("extra", EXTRAS)
def test_fail_two_shards_equal_one_handle(extra):
    cut = 36      # inside the first tile
    whole = _fail_env("hexa", "v2", 1, seed=13, fail=SOME, **extra)
    h0 = _fail_env("hexa", "v2", 1, cut, seed=13, fail=SOME, **extra)
    h1 = _fail_env("hexa", "v2", 1, N - cut, seed=13, fail=SOME, env_id_offset=cut, **extra)
    H.check_two_shards(whole, h0, h1, cut, _actions(T, N, 4, whole.device, wide=True), side=(SW,), every_step=True)
    for e in (whole, h0, h1):
        e.close()


@pytest.mark.parametrize("extra", EXTRAS)
def test_ppo_fused_rollout_with_rotor_failure(extra):
    H.check_ppo_fused_rollout_replays(SW, 4096, 16, rotor_failure=FAIL, **extra)


# ---- 6. the one-launch evaluation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,nwp,deterministic,extra", [("quad", 1, True, {}), ("hexa", 2, False, dict(randomization=WIDE)), ("hexa", 1, True, LDS)])
def test_fused_evaluation_with_rotor_failure_is_the_twin_rollout_reduced(vehicle, nwp, deterministic, extra):
    """tests/test_gpu_evaluate.py's method on 40 envs (16-env workgroups, the last one partial), 2 episodes each: counts identical, returns bit-equal."""
    n, mes = 40, 30
    env = _fail_env(vehicle, "v2", nwp, n, max_episode_steps=mes, **extra)
    twin = _fail_env(vehicle, "v2", nwp, n, max_episode_steps=mes, block_size=64, **extra)
    _, c, steps, _ = check_against_twin(env, twin, lambda: H.policy(env.obs_dim), per_env=2, max_steps=2 * (mes + 2), deterministic=deterministic)
    assert bool((c[:, 0] == 2).all()) and steps <= 2 * (mes + 1)
    env.close(); twin.close()


# ---- 7. refusals and re-keying ----------------------------------------------------------------------------------------------------------
def _raw(env, **kw):
    c = FAIL.to_c()
    for k, v in kw.items():
        setattr(c, k, v)
    return env.lib.amenv_set_rotor_failure(env._h, C.byref(c))


def test_fail_refusals_leave_everything_untouched():
    def asks(env):
        with pytest.raises(L.AmenvError):
            env.set_rotor_failure(FAIL)
        with pytest.raises(L.AmenvError):
            env.rotor_failure_state()

    H.check_refused(SW, lambda: _env("hexa_arm", "v2", 1, 64), asks)
    with pytest.raises(L.AmenvError):
        _env("hexa_arm", "v2", 1, 64, n_joints=2, rotor_failure=FAIL)
    H.check_refused(SW, lambda: amd.GpuWaypointEnv(64, config=H.octo_config(64)), FAIL, "4 or 6 rotors")
    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64, kernel="team"), FAIL, "lane-quad")
    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64), amd.RotorFailure(rotors=[1, 4]), "4 rotors")

    def bad_values(env):      # through ctypes: the C ABI's own checks
        inf, nan = float("inf"), float("nan")
        err = lambda: env.lib.amenv_last_error(env._h)
        assert _raw(env, struct_size=24) == -1 and b"struct_size" in err()
        for bad in (nan, inf, -inf, -0.01, 1.01):
            assert _raw(env, probability=bad) == -1 and b"probability" in err(), bad
        for lo, hi in [(-1, 5), (6, 5), (0, 65536), (70000, 70001)]:
            assert _raw(env, onset_min=lo, onset_max=hi) == -1 and b"onset" in err(), (lo, hi)
        for lo, hi in [(-0.1, 0.5), (0.6, 0.5), (0.0, 1.1), (nan, 0.5), (0.0, nan), (0.0, inf)]:
            assert _raw(env, remaining_min=lo, remaining_max=hi) == -1 and b"remaining" in err(), (lo, hi)
        for mask in (1 << 4, 0b110000, 1 << 31):
            assert _raw(env, rotor_mask=mask) == -1 and b"rotor_mask" in err(), mask
        assert env.lib.amenv_rotor_failure_state(env._h, None, None, None) == -1
        with pytest.raises(L.AmenvError, match="off"):
            env.rotor_failure_state()

    H.check_refused(SW, lambda: _env("quad", "v2", 1, 64), bad_values)
    env = _fail_env("quad", "v2", 1, 64, fail=SOME)        # a refusal on a handle where it is on keeps the old values
    env.reset()
    before = [x.clone() for x in env.rotor_failure_state()]
    assert _raw(env, probability=2.0) == -1 and _raw(env, rotor_mask=1 << 4) == -1
    assert env.kernel_name.endswith(" +fail") and env.rotor_failure is SOME
    H.same_tensors(before, env.rotor_failure_state())
    plan = torch.empty(64, 2, dtype=torch.int32, device=env.device)      # either output alone
    assert env.lib.amenv_rotor_failure_state(env._h, C.c_void_p(plan.data_ptr()), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(plan, before[0])
    env.set_rotor_failure(None)
    assert "+fail" not in env.kernel_name and env.rotor_failure is None
    env.close()


def test_reseed_changes_the_plans():
    env = _fail_env("hexa", "v2", 1, 512, seed=13, fail=SOME)
    env.reset()
    ep = env.get_state()[1][L.I_EPISODE].cpu().numpy()
    before = env.rotor_failure_state()[0].cpu().numpy()
    assert np.array_equal(before, fail_ref.plans_all(13, 0, ep, 6, SOME)[0])
    env.reseed(14)
    after = env.rotor_failure_state()[0].cpu().numpy()
    assert not np.array_equal(before, after)
    assert np.array_equal(after, fail_ref.plans_all(14, 0, ep, 6, SOME)[0])
    env.close()
    venv = amd.GpuVecEnv(num_envs=256, vehicle="hexa", rotor_failure=FAIL)   # passed through **env_kwargs
    assert venv.backend.kernel_name.endswith(" +fail") and venv.backend.rotor_failure is FAIL
    venv.backend.close()
