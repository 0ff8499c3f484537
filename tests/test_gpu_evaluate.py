"""One-launch policy evaluation (amenv_evaluate_policy) against the one-launch ROLLOUT on a twin handle that runs the
one-lane-per-env form: same seed, same config, T = max_steps steps into buffers, and a host reduction of dones / info_bits / rewards to what
the evaluation kernel counts.  counts are identical, returns bit-equal (fp64 sums over fp32 values in episode order), steps_run equals the
step at which the last env filled its quota.  Deterministic mode: the twin's policy has log_std = -120 (exp is exactly 0 in fp32, its raw
actions are the means); stochastic mode: the policy's own log_std and the same (seed, draw0)."""
import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import PPO, ActorCritic, evaluate_policy, reduce_evaluation
from tests import switch_harness as H

pytestmark = pytest.mark.gpu

DR = amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1))
SWITCH_VALUES = {"randomization": DR, "rotor_lag": amd.RotorLag(0.015, 0.04),
                 "sensor_noise": amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01), "action_delay": amd.ActionDelay(0, 8),
                 "action_history": amd.ActionHistory(2)}


# ---- the reference: the twin's rollout, reduced on the host ------------------------------------------------------------------------------
def host_reduction(rewards, dones, info, per_env, ret0, len0):
    """What the evaluation kernel counts, from T rollout rows: per env the first per_env episode ends; an episode's return is the sequential
    fp32 sum of its rewards (ep_return += reward), continued from (ret0, len0) for the episode running at entry.  Returns returns [N, 2] f64,
    counts [N, 6] i32, the number of steps after which no env was short of its quota (T if some still were) and how many counted episodes
    ended TRUNCATED without TERMINATED."""
    T, n = rewards.shape
    run, ln = ret0.astype(np.float32).copy(), len0.astype(np.int64).copy()
    returns, counts = np.zeros((n, 2)), np.zeros((n, L.EVAL_COUNT_COLS), dtype=np.int32)
    steps, cut_only = T, 0
    for t in range(T):
        run = (run + rewards[t]).astype(np.float32)
        ln += 1
        d = dones[t] != 0
        take = d & (counts[:, 0] < per_env)
        r = run[take].astype(np.float64)
        returns[take, 0] += r
        returns[take, 1] += r * r
        counts[take, 0] += 1
        counts[take, 1] += ln[take].astype(np.int32)
        for col, bit in ((2, L.INFO_SUCCESS), (3, L.INFO_CRASHED), (4, L.INFO_OOB), (5, L.INFO_TRUNCATED)):
            counts[take, col] += ((info[t][take] & bit) != 0).astype(np.int32)
        cut_only += int(((info[t][take] & (L.INFO_TERMINATED | L.INFO_TRUNCATED)) == L.INFO_TRUNCATED).sum())
        run[d], ln[d] = 0.0, 0
        if bool((counts[:, 0] >= per_env).all()):
            steps = t + 1
            break
    return returns, counts, steps, cut_only


def twin_rollout(twin, pol, T, seed, draw0, norm=None):
    n, dev = twin.num_envs, twin.device
    f, i = twin.get_state()
    ret0, len0 = f[L.F_EP_RETURN].cpu().numpy(), i[L.I_STEP].cpu().numpy()
    b = dict(obs=torch.empty(T + 1, n, twin.obs_dim, device=dev), actions=torch.empty(T, n, twin.act_dim, device=dev), logp=torch.empty(T, n, device=dev),
             values=torch.empty(T, n, device=dev), rewards=torch.empty(T, n, device=dev), dones=torch.empty(T, n, dtype=torch.uint8, device=dev))
    info = torch.zeros(T, n, dtype=torch.int32, device=dev)
    kw = {} if norm is None else dict(obs_normalizer=norm, update_normalizer=False)
    twin.rollout_policy(pol.flat_param, T, seed, draw0, info_bits=info, **b, **kw)
    torch.cuda.synchronize()
    return b["rewards"].cpu().numpy(), b["dones"].cpu().numpy(), info.cpu().numpy().view(np.uint32), ret0, len0


def frozen(make_policy):
    """The policy with log_std = -120: std = exp(-120) rounds to 0 in fp32, the sample IS the mean."""
    p = make_policy()
    with torch.no_grad():
        p.log_std.data.fill_(-120.0)
    return p


def fixture():
    return H.fixture_policy("cuda").flatten_()


def check_against_twin(env, twin, make_policy, per_env, max_steps, deterministic, norm=None, seed=21, draw0=7, reset=True):
    """env.evaluate_policy against the host reduction of twin's rollout.  Both handles stand at the same state.  Returns the arrays on the host, steps_run and the twin's count of time-limit-only ends."""
    pol = make_policy()
    out = env.evaluate_policy(pol.flat_param, per_env, max_steps=max_steps, deterministic=deterministic, seed=seed, draw0=draw0, obs_normalizer=norm, reset=reset)
    if reset:
        twin.reset()
    rw, dn, info, ret0, len0 = twin_rollout(twin, frozen(make_policy) if deterministic else pol, max_steps, seed, draw0, norm)
    want_r, want_c, want_steps, cut_only = host_reduction(rw, dn, info, per_env, ret0, len0)
    got_r, got_c, got_steps = out["returns"].cpu().numpy(), out["counts"].cpu().numpy(), int(out["steps_run"])
    assert out["returns"].dtype == torch.float64 and out["counts"].dtype == torch.int32 and out["steps_run"].dtype == torch.int32 and out["steps_run"].dim() == 0
    assert got_r.shape == (env.num_envs, 2) and got_c.shape == (env.num_envs, 6)
    assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:5]
    assert np.array_equal(got_r.view(np.uint64), want_r.view(np.uint64)), np.argwhere(got_r != want_r)[:5]
    assert got_steps == want_steps == min(max_steps, want_steps)
    return got_r, got_c, got_steps, cut_only


def quad_pair(n=300, seed=4, **kw):
    kw.setdefault("max_episode_steps", 200); kw.setdefault("counter_limit", 40)
    return amd.GpuWaypointEnv(n, seed=seed, **kw), amd.GpuWaypointEnv(n, seed=seed, block_size=64, **kw)


# ---- the checkpoint on the quadrotor: masking after the quota, early exit, step limit, a running episode ---------------------------------
@pytest.mark.parametrize("deterministic", [True, False])
def test_quadrotor_checkpoint_two_episodes_per_env(deterministic):
    env, twin = quad_pair()
    _, c, steps, cut_only = check_against_twin(env, twin, fixture, per_env=2, max_steps=500, deterministic=deterministic)
    k = c[:, 0].sum()
    assert k == 600 and bool((c[:, 0] == 2).all())
    if deterministic:   # conditions of the case (it exercises both kinds of end, the masking after the quota and the early exit)
        assert c[:, 2].sum() >= 0.1 * k and cut_only >= 0.1 * k, (c.sum(0), cut_only)      # SUCCESS | TRUNCATED without TERMINATED
    assert steps < 500
    env.close(); twin.close()


def test_quadrotor_checkpoint_step_limit_cuts_the_quota():
    env, twin = quad_pair()
    _, c, steps, _ = check_against_twin(env, twin, fixture, per_env=2, max_steps=250, deterministic=True)
    assert steps == 250 and bool((c[:, 0] < 2).any()) and c[:, 0].sum() > 0
    env.close(); twin.close()


def test_running_episode_counts_when_it_ends():
    env, twin = quad_pair()
    env.reset(); twin.reset()
    acts = H.actions(30, 300, 5, env.device)
    for t in range(30):
        env.step(acts[t])
    twin.set_state(*env.get_state())
    _, c, _, _ = check_against_twin(env, twin, fixture, per_env=1, max_steps=260, deterministic=True, reset=False)
    assert bool((c[:, 0] == 1).all()) and c[:, 1].max() > 200          # lengths include the 30 steps flown before the call
    env.close(); twin.close()


# ---- every form -----------------------------------------------------------------------------------------------------------------------------
def test_hexa_v1_raw_with_the_normaliser_frozen():
    n = 4096
    mk = lambda: amd.GpuWaypointEnv(n, vehicle="hexa", task="v1_raw", seed=6, max_episode_steps=60)   # noqa: E731
    env, twin, warm = mk(), mk(), mk()
    pol = lambda: H.policy(17)   # noqa: E731
    nrm = ObsNormalizer(17)
    warm.reset()
    nrm.update(warm.observe())
    b = H.buffers(20, n, 17, warm.device)
    warm.rollout_policy(pol().flat_param, 20, seed=1, draw0=0, obs_normalizer=nrm, update_normalizer=True, **b)   # warmed by one rollout
    before = [np.array(x, copy=True) for x in nrm.get()]
    _, c, _, _ = check_against_twin(env, twin, pol, per_env=1, max_steps=62, deterministic=False, norm=nrm)
    for x, y in zip(before, nrm.get()):
        assert np.array_equal(x.view(np.uint64), np.asarray(y).view(np.uint64))                  # the statistics, bit for bit
    assert c[:, 0].sum() == n
    for x in (env, twin, warm, nrm):
        x.close()


@pytest.mark.parametrize("vehicle,nwp,n,mes,deterministic", [("quad", 3, 12000, 60, True), ("hexa", 1, 40000, 25, False)])
def test_rigid_large_grids(vehicle, nwp, n, mes, deterministic):
    env = amd.GpuWaypointEnv(n, vehicle=vehicle, num_waypoints=nwp, seed=8, max_episode_steps=mes)
    twin = amd.GpuWaypointEnv(n, vehicle=vehicle, num_waypoints=nwp, seed=8, max_episode_steps=mes, block_size=64)
    _, c, _, _ = check_against_twin(env, twin, lambda: H.policy(20), per_env=1, max_steps=mes + 2, deterministic=deterministic)
    assert c[:, 0].sum() == n
    env.close(); twin.close()


def arm_policy(od, ad):
    def make():
        torch.manual_seed(11)
        p = ActorCritic(od, ad).cuda().flatten_()
        with torch.no_grad():
            p.log_std.data.fill_(-1.0)
            p.action_net.weight.mul_(20.0)
            p.action_net.bias[0] = 1.0
        return p
    return make


@pytest.mark.parametrize("nj,nwp,n,deterministic", [(3, 1, 300, True), (2, 3, 300, False), (3, 1, 20000, False)])
def test_hexa_arm(nj, nwp, n, deterministic):
    kw = dict(vehicle="hexa_arm", n_joints=nj, num_waypoints=nwp, seed=12, max_episode_steps=40)
    env, twin = amd.GpuWaypointEnv(n, **kw), amd.GpuWaypointEnv(n, kernel="lane", **kw)
    _, c, _, _ = check_against_twin(env, twin, arm_policy(env.obs_dim, env.act_dim), per_env=1, max_steps=42, deterministic=deterministic)
    assert c[:, 0].sum() == n
    env.close(); twin.close()


@pytest.mark.parametrize("sw", [H.RANDOMIZATION, H.ROTOR_LAG, H.SENSOR_NOISE, H.ACTION_DELAY, H.ACTION_HISTORY], ids=lambda s: s.kw)
@pytest.mark.parametrize("deterministic", [True, False])
def test_every_switch(sw, deterministic):
    kw = {sw.kw: SWITCH_VALUES[sw.kw]}
    env, twin = H.make_env("quad", "v2", 1, 300, **kw), H.make_env("quad", "v2", 1, 300, block_size=64, **kw)
    assert sw.suffix in env.kernel_name
    _, c, _, _ = check_against_twin(env, twin, lambda: H.policy(env.obs_dim), per_env=2, max_steps=54, deterministic=deterministic)
    assert c[:, 0].sum() == 600
    env.close(); twin.close()


def test_all_switches_with_the_normaliser():
    kw = {k: v for k, v in SWITCH_VALUES.items() if k != "action_history"}
    mk = lambda **x: H.make_env("hexa", "v1_scaled", 1, 300, **kw, **x)   # noqa: E731
    env, twin = mk(), mk()
    nrm = ObsNormalizer(17)
    twin.reset()
    nrm.update(env.reset())                                      # (both handles stand at their first reset: no second one, which would start other episodes)
    check_against_twin(env, twin, lambda: H.policy(17), per_env=1, max_steps=27, deterministic=True, norm=nrm, reset=False)
    for x in (env, twin, nrm):
        x.close()


# ---- side effects, determinism, shards ---------------------------------------------------------------------------------------------------
def test_monitor_totals_untouched_and_the_handle_stays_usable():
    env, fresh = (amd.GpuWaypointEnv(300, seed=4, max_episode_steps=25, counter_limit=40) for _ in range(2))
    env.reset()
    acts = H.actions(8, 300, 3, env.device)
    for t in range(4):
        env.step(acts[t])
    before = env.stats()
    out = env.evaluate_policy(fixture().flat_param, 2, reset=False)
    torch.cuda.synchronize()
    assert env.stats() == before and before["steps"] == 4 * 300
    assert int(out["counts"][:, 0].sum()) == 600
    # wherever its lanes stopped, the state in the blob is whole: after reset() a fresh handle given that state steps like it, bit for bit
    env.reset()
    _, i = env.get_state()
    assert int(i[L.I_EPISODE].min()) >= 2 and int(i[L.I_STEP].max()) == 0
    fresh.reset()
    fresh.set_state(*env.get_state())
    assert torch.equal(env.observe(), fresh.observe())
    for t in range(4, 8):
        ra, da = H.step_all(env, acts[t]); rb, db = H.step_all(fresh, acts[t])
        H.same_step(ra, da, rb, db, t)
    H.same_state(env, fresh)
    env.close(); fresh.close()


def test_two_calls_on_twin_handles_agree_exactly():
    a, b = (amd.GpuWaypointEnv(1000, vehicle="hexa", seed=5, max_episode_steps=30) for _ in range(2))
    pol = H.policy(20)
    oa = a.evaluate_policy(pol.flat_param, 2, deterministic=False, seed=3, draw0=11)
    ob = b.evaluate_policy(pol.flat_param, 2, deterministic=False, seed=3, draw0=11)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    H.same_state(a, b)
    oc = a.evaluate_policy(pol.flat_param, 2, deterministic=False, seed=4, draw0=11)
    assert not torch.equal(oa["returns"], oc["returns"])               # (another key: other noise)
    a.close(); b.close()


def test_two_shards_concatenate_to_the_whole():
    n, cut = 300, 112
    kw = dict(seed=9, max_episode_steps=30, num_waypoints=2)
    whole, h0, h1 = amd.GpuWaypointEnv(n, **kw), amd.GpuWaypointEnv(cut, **kw), amd.GpuWaypointEnv(n - cut, env_id_offset=cut, **kw)
    pol = H.policy(20)
    ow, o0, o1 = (e.evaluate_policy(pol.flat_param, 2, deterministic=False, seed=3, draw0=2) for e in (whole, h0, h1))
    assert torch.equal(ow["returns"], torch.cat([o0["returns"], o1["returns"]])) and torch.equal(ow["counts"], torch.cat([o0["counts"], o1["counts"]]))
    assert int(ow["steps_run"]) == max(int(o0["steps_run"]), int(o1["steps_run"]))
    for e in (whole, h0, h1):
        e.close()


# ---- refusals: the error, and the handle as it was ------------------------------------------------------------------------------------------
_ASKED = H.Switch("randomization", "+evaluated", "set_randomization", lambda e: ())   # (check_refused wants a switch: one that none of these handles has)


def _ask(match, norm_dim=None, **kw):
    def what(env):
        nrm = None if norm_dim is None else ObsNormalizer(norm_dim)
        pol = H.policy(env.obs_dim) if env.act_dim == 4 else arm_policy(env.obs_dim, env.act_dim)()
        args = dict(episodes_per_env=1, max_steps=10, reset=False, obs_normalizer=nrm)
        args.update(kw)
        with pytest.raises(L.AmenvError, match=match):
            env.evaluate_policy(pol.flat_param, args.pop("episodes_per_env"), **args)
        if nrm is not None:
            nrm.close()
    return what


def _null_pointers(env):
    pol = H.policy(env.obs_dim)
    outs = [torch.zeros(64, dtype=torch.float64, device=env.device) for _ in range(3)]
    ok = [env._h, None, 0.0, 0.0, pol.flat_param.data_ptr(), 1, 0, 0, 1, 10] + [t.data_ptr() for t in outs] + [None]
    for k in (4, 10, 11, 12):
        a = list(ok); a[k] = None
        assert env.lib.amenv_evaluate_policy(*a) == -1 and b"non-NULL" in env.lib.amenv_last_error(env._h)
    assert env.lib.amenv_evaluate_policy(None, *ok[1:]) == -1


REFUSALS = {
    "null_pointers": (lambda: H.make_env("quad", "v2", 1, 8), _null_pointers),
    "no_episodes": (lambda: H.make_env("quad", "v2", 1, 70), _ask("must be > 0", episodes_per_env=0)),
    "no_steps": (lambda: H.make_env("quad", "v2", 1, 70), _ask("must be > 0", max_steps=0)),
    "fp64": (lambda: H.make_env("quad", "v2", 1, 70, dtype="f64"), _ask("fp32 handles")),
    "no_auto_reset": (lambda: H.make_env("hexa", "v2", 2, 70, auto_reset=False), _ask("AMENV_FLAG_AUTO_RESET")),
    "eight_rotors": (lambda: amd.GpuWaypointEnv(70, config=H.octo_config(70)), _ask("4 or 6 rotors")),
    "normaliser_on_an_arm": (lambda: H.make_env("hexa_arm", "v2", 1, 70), _ask("rigid vehicles", norm_dim=29)),
    "normaliser_dim": (lambda: H.make_env("quad", "v2", 1, 70), _ask("dim differs", norm_dim=17)),
    "normaliser_with_history": (lambda: H.make_env("quad", "v2", 1, 70, action_history=amd.ActionHistory(1)), _ask("action history", norm_dim=20)),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refused_before_anything_is_launched(case):
    make, what = REFUSALS[case]
    H.check_refused(_ASKED, make, what)


# ---- amd.evaluate_policy(fused=True) and PPO.learn ---------------------------------------------------------------------------------------------
def test_fused_evaluate_policy_is_the_host_reduction_and_the_checkpoint_succeeds():
    n = 4096
    env, twin = amd.GpuWaypointEnv(n, seed=3), amd.GpuWaypointEnv(n, seed=3)
    pol = fixture()
    mean, std, info = evaluate_policy(pol, env, n_eval_episodes=n, fused=True, return_info=True)
    out = twin.evaluate_policy(pol.flat_param, 1)
    m2, s2, i2 = reduce_evaluation(out["returns"], out["counts"], int(out["steps_run"]))
    assert (mean, std, info) == (m2, s2, i2)
    two = evaluate_policy(pol, env, n_eval_episodes=n, fused=True)          # (the env's next episodes: other start states, other numbers)
    assert len(two) == 2 and all(isinstance(x, float) for x in two)
    assert info["episodes"] == n and info["success_rate"] > 0.95, info
    assert 0 < info["steps_run"] <= int(env.cfg.task.max_episode_steps) + 2
    # recorded, not gated: the fused (bf16 behaviour policy) mean against the step-by-step fp32 one, in units of the latter's standard error
    m_ref, s_ref = evaluate_policy(pol, env, n_eval_episodes=n)
    print(f"fused mean {mean:.3f} (std {std:.3f}), step-by-step {m_ref:.3f} (std {s_ref:.3f}): {(mean - m_ref) / (s_ref / np.sqrt(n)):+.2f} standard errors; info {info}")
    with pytest.raises(L.AmenvError, match="no episode finished"):
        evaluate_policy(pol, env, n_eval_episodes=n, fused=True, max_steps=3)
    env.close(); twin.close()


def test_ppo_learn_with_eval_env_leaves_training_bit_identical(tmp_path):
    def run(with_eval):
        env = amd.GpuWaypointEnv(256, seed=2, max_episode_steps=40)
        model = PPO(env, n_steps=16, batch_size=1024, n_epochs=2, seed=1, fused_rollout=True)
        kw = {}
        if with_eval:
            kw = dict(eval_env=amd.GpuWaypointEnv(256, seed=1002, max_episode_steps=40), eval_freq=16 * 256, best_model_save_path=str(tmp_path / "best"))
        model.learn(2 * 16 * 256, **kw)
        log, draw, gen = model.log, model._draw, model._gen.get_state().clone()
        env.close()
        if with_eval:
            kw["eval_env"].close()
        return log, draw, gen, model.policy.flat_param.detach().clone()
    (la, da, ga, pa), (lb, db, gb, pb) = run(False), run(True)
    assert len(la) == len(lb) == 2
    for a, b in zip(la, lb):
        assert {"eval_mean_reward", "eval_std_reward", "eval_success_rate", "eval_ep_len_mean"} <= set(b) and np.isfinite([b[k] for k in b if k.startswith("eval_")]).all()
        assert {k: v for k, v in b.items() if not k.startswith("eval_")} == a
    assert (tmp_path / "best" / "best_model.zip").exists()
    assert da == db and torch.equal(ga, gb) and torch.equal(pa, pb)
    with pytest.raises(L.AmenvError, match="separate GpuWaypointEnv"):
        env = amd.GpuWaypointEnv(64, seed=2)
        try:
            PPO(env, n_steps=4, batch_size=64, fused_rollout=True).learn(256, eval_env=env, eval_freq=256)
        finally:
            env.close()
