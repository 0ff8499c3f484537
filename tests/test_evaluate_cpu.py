"""One-launch evaluation, the host side: the reduction from amenv_evaluate_policy's two arrays to (mean, std, info), its
agreement with the step-by-step `evaluate_policy` on the oracle-backed stand-in, and `PPO.learn`'s evaluation bookkeeping with a stub in
place of the fused call.  No GPU."""
import math
import os
import types

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd import ppo as P
from rl_aerial_manipulator_amd.ppo import ActorCritic, evaluate_policy, reduce_evaluation
from tests.oracle_backend import OracleBackend
from tests.test_ppo_controls_cpu import _StandInEnv, _gae, _gaussian_act


# ---- the reduction ----------------------------------------------------------------------------------------------------------------------
def _arrays(episodes):
    """episodes: per env a list of (return, length, success, crashed, oob, truncated) -> the two arrays, built as the kernel builds them"""
    n = len(episodes)
    returns, counts = np.zeros((n, 2)), np.zeros((n, 6), dtype=np.int32)
    for i, eps in enumerate(episodes):
        for r, ln, *flags in eps:
            r = float(np.float32(r))
            returns[i] += (r, r * r)
            counts[i] += np.array([1, ln, *flags], dtype=np.int32)
    return returns, counts


def test_reduction_matches_numpy_on_hand_made_arrays():
    eps = [[(10.5, 40, 1, 0, 0, 0), (-3.25, 200, 0, 0, 0, 1)],
           [],                                                   # an env that finished nothing within the step limit
           [(7.0, 12, 0, 1, 1, 0)],                              # flags are not exclusive: crashed and out of bounds
           [(1e-3, 200, 0, 0, 0, 1), (250.0, 33, 1, 0, 0, 0), (-80.125, 5, 0, 1, 0, 0)]]
    returns, counts = _arrays(eps)
    mean, std, info = reduce_evaluation(returns, counts, steps_run=417)
    flat = np.array([float(np.float32(e[0])) for env in eps for e in env])
    assert mean == pytest.approx(flat.mean(), rel=1e-14) and std == pytest.approx(flat.std(), rel=1e-12)
    assert info["episodes"] == 6 and info["steps_run"] == 417
    assert info["ep_len_mean"] == pytest.approx((40 + 200 + 12 + 200 + 33 + 5) / 6)
    assert info["success_rate"] == pytest.approx(2 / 6) and info["crash_rate"] == pytest.approx(2 / 6)
    assert info["oob_rate"] == pytest.approx(1 / 6) and info["truncated_rate"] == pytest.approx(2 / 6)
    # tensors are taken too, and steps_run may be left out
    m2, s2, i2 = reduce_evaluation(torch.from_numpy(returns), torch.from_numpy(counts))
    assert (m2, s2) == (mean, std) and i2["steps_run"] is None and {k: v for k, v in i2.items() if k != "steps_run"} == {k: v for k, v in info.items() if k != "steps_run"}


def test_reduction_of_one_episode_has_zero_std_and_never_a_negative_variance():
    returns, counts = _arrays([[(123.456, 7, 1, 0, 0, 0)], []])
    mean, std, info = reduce_evaluation(returns, counts)
    assert mean == float(np.float32(123.456)) and std == 0.0 and info["episodes"] == 1
    returns[0, 1] *= 1 - 1e-15                                   # rounding may leave E[r^2] a hair below mean^2
    assert reduce_evaluation(returns, counts)[1] == 0.0


def test_reduction_raises_when_nothing_was_counted():
    with pytest.raises(L.AmenvError, match="no episode finished"):
        reduce_evaluation(np.zeros((5, 2)), np.zeros((5, 6), dtype=np.int32), steps_run=100)


# ---- against the existing evaluate_policy on the oracle -----------------------------------------------------------------------------------
class _OracleEvalEnv:
    """What `evaluate_policy` touches of a GpuWaypointEnv, on the CPU oracle."""

    def __init__(self, n, seed, max_episode_steps):
        self.b = OracleBackend(n, seed=seed, max_episode_steps=max_episode_steps)
        self.num_envs, self.cfg = n, self.b.cfg
        self.ep_return, self.ep_len = self.b.ep_return, self.b.ep_len
        self.trace = []

    def reset(self):
        return self.b.reset().to(torch.float32)

    def step(self, actions):
        o, r, d, info = self.b.step(actions.numpy())
        self.trace.append((d.numpy().astype(bool).copy(), self.b.ep_return.numpy().copy(), self.b.ep_len.numpy().copy(), info.numpy().view(np.uint32).copy()))
        return o.to(torch.float32), r, d, info


def test_reduction_of_per_env_sums_equals_the_step_by_step_evaluation():
    torch.manual_seed(5)
    pol = ActorCritic(20, 4)
    with torch.no_grad():
        pol.action_net.bias.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))   # near hover: episodes run into the time limit, some drift out
    n, per_env = 24, 2
    env = _OracleEvalEnv(n, seed=4, max_episode_steps=30)
    mean, std = evaluate_policy(pol, env, n_eval_episodes=n * per_env, deterministic=True, check_every=1)
    # the kernel's accounting, replayed on the host from the same steps
    returns, counts = np.zeros((n, 2)), np.zeros((n, 6), dtype=np.int32)
    for done, ep_ret, ep_len, bits in env.trace:
        for i in np.nonzero(done)[0]:
            if counts[i, 0] < per_env:
                r = float(ep_ret[i])
                returns[i] += (r, r * r)
                counts[i] += np.array([1, ep_len[i]] + [int(bool(bits[i] & b)) for b in (L.INFO_SUCCESS, L.INFO_CRASHED, L.INFO_OOB, L.INFO_TRUNCATED)], dtype=np.int32)
    m2, s2, info = reduce_evaluation(returns, counts, steps_run=len(env.trace))
    assert info["episodes"] == n * per_env
    assert m2 == pytest.approx(mean, abs=1e-12, rel=1e-12) and s2 == pytest.approx(std, abs=1e-12, rel=1e-12)
    assert 0.0 <= info["success_rate"] <= 1.0 and info["ep_len_mean"] <= 30 + 2 and std > 0.0


def test_default_path_refuses_return_info_and_fused_needs_flat_parameters():
    env = _OracleEvalEnv(4, seed=1, max_episode_steps=10)
    with pytest.raises(L.AmenvError, match="return_info needs fused=True"):
        evaluate_policy(ActorCritic(20, 4), env, return_info=True)
    with pytest.raises(L.AmenvError, match="flat_param"):
        evaluate_policy(types.SimpleNamespace(predict=lambda o, d: o), env, fused=True)


# ---- PPO.learn's bookkeeping ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_rollout(monkeypatch):
    monkeypatch.setattr(P, "gaussian_act", _gaussian_act)
    monkeypatch.setattr(P, "compute_gae", _gae)


def _model(seed=1):
    return amd.PPO(_StandInEnv(8), n_steps=4, batch_size=16, n_epochs=2, seed=seed, use_graph=False, fused_mlp=False, bootstrap_truncated=False)


def _stub(monkeypatch, means):
    """In place of the fused call: hands out `means` in turn and records who asked."""
    calls = []

    def fake(model, env, n_eval_episodes, deterministic, max_steps, seed=0, draw0=0):
        calls.append(dict(timesteps=model.num_timesteps, env=env, n=n_eval_episodes, deterministic=deterministic, draw=model._draw,
                          gen=model._gen.get_state().clone()))
        m = means[len(calls) - 1]
        return m, 1.5, dict(episodes=n_eval_episodes, ep_len_mean=21.0, success_rate=0.25, crash_rate=0.0, oob_rate=0.0, truncated_rate=0.75, steps_run=30)
    monkeypatch.setattr(P, "_evaluate_fused", fake)
    return calls


def _eval_env(n=5, seed=9):
    return types.SimpleNamespace(num_envs=n, cfg=types.SimpleNamespace(seed=seed))


def test_learn_evaluates_by_the_save_freq_rule_and_saves_on_strict_improvement_only(cpu_rollout, monkeypatch, tmp_path):
    model = _model()
    saved = []
    monkeypatch.setattr(model, "save", lambda path: saved.append((path, model.num_timesteps, model.best_mean_reward)))
    calls = _stub(monkeypatch, [3.0, 3.0, 2.0, 7.5])
    ev = _eval_env()
    # 32 env steps per iteration; eval_freq 48: multiples 48, 96, 144, 192 -> the boundaries at 64, 96, 160, 192
    model.learn(6 * 32, eval_env=ev, eval_freq=48, eval_deterministic=False, best_model_save_path=str(tmp_path / "best"))
    assert [c["timesteps"] for c in calls] == [64, 96, 160, 192]
    assert all(c["env"] is ev and c["n"] == 5 and c["deterministic"] is False for c in calls)   # default: one episode per eval env
    with_eval = [r["timesteps"] for r in model.log if "eval_mean_reward" in r]
    assert with_eval == [64, 96, 160, 192] and len(model.log) == 6
    rec = model.log[1]
    assert (rec["eval_mean_reward"], rec["eval_std_reward"], rec["eval_success_rate"], rec["eval_ep_len_mean"]) == (3.0, 1.5, 0.25, 21.0)
    assert "eval_scope" not in rec
    # 3.0 (first), 3.0 (equal: no), 2.0 (worse: no), 7.5 (better)
    assert [(os.path.basename(p), t, b) for p, t, b in saved] == [("best_model", 64, 3.0), ("best_model", 192, 7.5)]
    assert all(os.path.dirname(p) == str(tmp_path / "best") for p, _, _ in saved) and os.path.isdir(tmp_path / "best")
    assert model.best_mean_reward == 7.5
    # a second learn() keeps the best so far and continues the multiples from where the job stands
    calls2 = _stub(monkeypatch, [7.5, 8.0])
    model.learn(2 * 32, eval_env=ev, eval_freq=48, n_eval_episodes=11, best_model_save_path=str(tmp_path / "best"))
    assert [c["timesteps"] for c in calls2] == [256] and calls2[0]["n"] == 11 and len(saved) == 2


def test_learn_refuses_the_training_env_and_half_an_evaluation_setup(cpu_rollout):
    model = _model()
    with pytest.raises(L.AmenvError, match="separate GpuWaypointEnv"):
        model.learn(32, eval_env=model.env, eval_freq=32)
    with pytest.raises(L.AmenvError, match="go together"):
        model.learn(32, eval_env=_eval_env())
    with pytest.raises(L.AmenvError, match="go together"):
        model.learn(32, eval_freq=32)
    assert model.num_timesteps == 0 and model.log == []


def test_evaluation_leaves_the_training_log_the_generator_and_the_draw_counter_alone(cpu_rollout, monkeypatch):
    plain = _model()
    plain.learn(4 * 32)
    model = _model()
    real = P._evaluate_fused
    seen = []

    def fake(m, env, n_eval_episodes, deterministic, max_steps, seed=0, draw0=0):
        seen.append((seed, draw0))
        return 1.0, 0.0, dict(episodes=1, ep_len_mean=1.0, success_rate=0.0, crash_rate=0.0, oob_rate=0.0, truncated_rate=1.0, steps_run=1)
    monkeypatch.setattr(P, "_evaluate_fused", fake)
    before = []
    inner = model._evaluate

    def spy(*a):
        g0, d0 = model._gen.get_state().clone(), model._draw
        out = inner(*a)
        before.append(torch.equal(g0, model._gen.get_state()) and d0 == model._draw)
        return out
    model._evaluate = spy
    model.learn(4 * 32, eval_env=_eval_env(seed=77), eval_freq=32)
    assert real is not fake and before == [True] * 4 and seen == [(77, 0)] * 4      # its own key: the eval env's seed, never the trainer's counter
    assert len(plain.log) == len(model.log) == 4
    for a, b in zip(plain.log, model.log):
        assert {k: v for k, v in b.items() if not k.startswith("eval_")} == a     # every training figure, bit for bit
        assert all(math.isfinite(v) for v in a.values())
    assert torch.equal(plain.policy.flat_param, model.policy.flat_param) and plain._draw == model._draw
    assert torch.equal(plain._gen.get_state(), model._gen.get_state())


def test_every_rank_evaluates_its_own_shard_and_says_so(cpu_rollout, monkeypatch):
    model = _model()
    model.world = 2                                              # (what PPO reads of `dist` when it tags the record)
    _stub(monkeypatch, [1.0])
    model.learn(32, eval_env=_eval_env(), eval_freq=32)
    assert model.log[0]["eval_scope"] == "rank"
