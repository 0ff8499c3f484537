"""PPO training controls on the host paths: SB3's target_kl early stop and approx_kl on the torch update path against a
literal restatement of SB3 2.6.0 `PPO.train`, learning-rate / clip-range schedules through `PPO.learn` on the oracle-backed stand-in
env, explained_variance, what is refused, the checkpoint fields.  No GPU."""
import copy
import math
import types

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import ppo as P
from rl_aerial_manipulator_amd.ppo import ActorCritic, MinibatchStep, explained_variance, ppo_update
from tests.oracle_backend import OracleBackend

N, BATCH, EPOCHS = 1000, 250, 3          # 4 minibatches x 3 epochs
LR = 3e-3                                 # large enough that approx_kl grows from minibatch to minibatch


def _policy_pair(seed=1):
    torch.manual_seed(seed)
    a = ActorCritic(20, 4)
    b = copy.deepcopy(a)
    a.flatten_()
    leaf = a.flat_param.requires_grad_(True)
    leaf.grad = a.flat_grad
    return a, torch.optim.Adam([leaf], lr=LR, eps=1e-5), b, torch.optim.Adam(b.parameters(), lr=LR, eps=1e-5)


def _rollout_like(pol, n, seed=0):
    """Rollout-shaped data: old log-probs are the policy's own (approx_kl starts at 0 and grows with the update)."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, 20, generator=g)
    with torch.no_grad():
        actions = pol.actor(obs) + torch.randn(n, 4, generator=g)
        _, old_logp, _ = pol.evaluate_actions(obs, actions)
    adv = torch.randn(n, generator=g) * 3.0 + 1.0
    ret = torch.randn(n, generator=g) * 10.0
    return obs, actions, old_logp.clone(), adv, ret


def _sb3_train(pol, opt, data, gen_seed, target_kl, clip=0.2, ent=5e-4, vf=0.5, max_norm=0.5):
    """SB3 2.6.0 PPO.train, restated: per epoch one permutation, per minibatch loss -> approx_kl -> (break) -> optimiser step."""
    obs, actions, old_logp, adv_all, ret = data
    gen = torch.Generator().manual_seed(gen_seed)
    kls, applied, continue_training = [], 0, True
    for _ in range(EPOCHS):
        perm = torch.randperm(N, generator=gen)
        for start in range(0, N, BATCH):
            idx = perm[start:start + BATCH]
            adv = adv_all[idx]
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            dist = torch.distributions.Normal(pol.actor(obs[idx]), pol.log_std.exp())
            logp = dist.log_prob(actions[idx]).sum(-1)
            ratio = (logp - old_logp[idx]).exp()
            pl = -torch.min(adv * ratio, adv * ratio.clamp(1 - clip, 1 + clip)).mean()
            vl = ((ret[idx] - pol.critic(obs[idx])) ** 2).mean()
            el = -dist.entropy().sum(-1).mean()
            with torch.no_grad():
                log_ratio = logp - old_logp[idx]
                kls.append(float(((log_ratio.exp() - 1) - log_ratio).mean()))
            if target_kl is not None and kls[-1] > 1.5 * target_kl:
                continue_training = False
                break
            opt.zero_grad()
            (pl + ent * el + vf * vl).backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), max_norm)
            opt.step()
            applied += 1
        if not continue_training:
            break
    return kls, applied


def _trip_point(kls):
    """A minibatch j of the second epoch whose approx_kl exceeds every earlier one by >= 1.2, and the limit halfway (geometric mean)
    between it and that running maximum: the stop cannot move to a neighbour by rounding."""
    for j in range(4, 8):
        top = max(kls[:j])
        if top > 0 and kls[j] >= 1.2 * top:
            return j, math.sqrt(kls[j] * top)
    raise AssertionError(f"test data: no minibatch of the second epoch tops the earlier ones by 1.2x: {kls}")


def test_torch_path_target_kl_stops_where_sb3_stops():
    a, opt_a, b, opt_b = _policy_pair()
    data = _rollout_like(b, N)
    probe = copy.deepcopy(b)                 # an ungated run records the approx_kl sequence the limit is placed in
    kls, applied_all = _sb3_train(probe, torch.optim.Adam(probe.parameters(), lr=LR, eps=1e-5), data, 7, None)
    assert applied_all == 12 and len(kls) == 12
    j, limit = _trip_point(kls)
    target_kl = limit / 1.5
    ref_kls, ref_applied = _sb3_train(b, opt_b, data, 7, target_kl)
    assert len(ref_kls) == j + 1 and ref_applied == j
    rec = ppo_update(a, opt_a, *data, batch_size=BATCH, n_epochs=EPOCHS, generator=torch.Generator().manual_seed(7), target_kl=target_kl)
    assert rec["n_updates"] == ref_applied and rec["kl_early_stop"] == 1
    assert rec["approx_kl"] == pytest.approx(np.mean(ref_kls), rel=1e-4)
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.allclose(va, vb, rtol=1e-5, atol=1e-7), k
    assert all(math.isfinite(v) for v in rec.values())


def test_torch_path_without_a_trip_runs_every_minibatch_and_reports_last_epoch_kl():
    a, opt_a, b, opt_b = _policy_pair()
    data = _rollout_like(b, N)
    kls, applied = _sb3_train(b, opt_b, data, 7, None)
    rec = ppo_update(a, opt_a, *data, batch_size=BATCH, n_epochs=EPOCHS, generator=torch.Generator().manual_seed(7))
    assert rec["n_updates"] == applied == 12 and rec["kl_early_stop"] == 0
    assert rec["approx_kl"] == pytest.approx(np.mean(kls[-4:]), rel=1e-4)          # target_kl=None: the last epoch's mean, like the losses
    a2, opt_a2, _, _ = _policy_pair()
    rec2 = ppo_update(a2, opt_a2, *data, batch_size=BATCH, n_epochs=EPOCHS, generator=torch.Generator().manual_seed(7), target_kl=1e9)
    assert torch.equal(a2.flat_param, a.flat_param) and rec2["n_updates"] == 12 and rec2["kl_early_stop"] == 0
    assert rec2["approx_kl"] == pytest.approx(np.mean(kls), rel=1e-4)              # with target_kl: over every evaluated minibatch


def test_explained_variance_is_sb3s_and_zero_on_constant_returns():
    g = np.random.default_rng(3)
    y = g.normal(size=(16, 8)).astype(np.float32) * 5 + 2
    v = (0.7 * y + g.normal(size=y.shape)).astype(np.float32)
    want = 1.0 - np.var(y.astype(np.float64) - v.astype(np.float64)) / np.var(y.astype(np.float64))
    got = explained_variance(torch.from_numpy(v), torch.from_numpy(y))
    assert got.dim() == 0 and float(got) == pytest.approx(want, rel=1e-6)
    assert float(explained_variance(torch.from_numpy(v), torch.full((16, 8), 3.0))) == 0.0     # SB3: NaN; a record stays finite
    assert float(explained_variance(torch.from_numpy(y), torch.from_numpy(y))) == 1.0


class _Dist2:
    def get_world_size(self):
        return 2

    def get_rank(self):
        return 0


def test_target_kl_refuses_captured_graphs_and_several_ranks():
    pol = ActorCritic(20, 4).flatten_()
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-4)
    with pytest.raises(amd.AmenvError, match="use_graph"):
        MinibatchStep(pol, opt, use_graph=True, target_kl=0.01)
    with pytest.raises(amd.AmenvError, match="ranks"):
        MinibatchStep(pol, opt, dist=_Dist2(), target_kl=0.01)
    with pytest.raises(amd.AmenvError, match="ranks"):
        amd.PPO(_StandInEnv(2), dist=_Dist2(), target_kl=0.01)
    with pytest.raises(amd.AmenvError, match="use_graph"):
        amd.PPO(_StandInEnv(2), use_graph=True, target_kl=0.01)
    with pytest.raises(amd.AmenvError, match="positive"):
        MinibatchStep(pol, opt, target_kl=0.0)
    assert MinibatchStep(pol, opt, target_kl=0.01).use_graph is False


# ---- PPO.learn on the CPU: the oracle-backed stand-in env, with torch restatements of the two HIP pieces of the rollout --------------
class _StandInEnv:
    state_dtype = torch.float32

    def __init__(self, n, seed=3):
        self.b = OracleBackend(n, seed=seed)
        self.num_envs, self.obs_dim, self.act_dim, self.device = n, self.b.obs_dim, 4, torch.device("cpu")
        self.cfg = types.SimpleNamespace(env_id_offset=0, vehicle=types.SimpleNamespace(n_joints=0))
        self.info_bits = torch.zeros(n, dtype=torch.int32)
        self.terminal_obs = self.b.terminal_obs
        self._ep = dict(episodes=0, return_sum=0.0, length_sum=0.0, success=0)

    def reset(self):
        return self.b.reset().to(torch.float32)

    def step_into(self, actions, obs_out, rew_out, done_out):
        o, r, d, info = self.b.step(actions.numpy())
        obs_out.copy_(o.to(torch.float32)); rew_out.copy_(r.to(torch.float32)); done_out.copy_(d.to(torch.uint8))
        self.info_bits = info
        m = d.to(torch.bool)
        self._ep["episodes"] += int(m.sum())
        self._ep["return_sum"] += float(self.b.ep_return[m].sum())
        self._ep["length_sum"] += float(self.b.ep_len[m].sum())

    def stats(self, reset=False):
        s = dict(self._ep)
        if reset:
            self._ep = dict(episodes=0, return_sum=0.0, length_sum=0.0, success=0)
        return s


def _gaussian_act(mean, log_std, low, high, raw_out, clipped_out, logp_out, seed, draw, env_id_offset=0):
    z = torch.randn(mean.shape, generator=torch.Generator().manual_seed(int(seed) * 7919 + int(draw)))
    raw_out.copy_(mean + log_std.exp() * z)
    clipped_out.copy_(torch.minimum(torch.maximum(raw_out, low), high))
    logp_out.copy_((-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi)).sum(-1))


def _gae(b, gamma, lam):
    a, nv = torch.zeros(b.n_envs), b.last_values
    for t in reversed(range(b.n_steps)):
        nnt = 1.0 - b.dones[t].to(torch.float32)
        delta = b.rewards[t] + gamma * nv * nnt - b.values[t]
        a = delta + gamma * lam * nnt * a
        b.advantages[t], b.returns[t], nv = a, a + b.values[t], b.values[t]
    return b.advantages, b.returns


@pytest.fixture
def cpu_rollout(monkeypatch):
    monkeypatch.setattr(P, "gaussian_act", _gaussian_act)
    monkeypatch.setattr(P, "compute_gae", _gae)


def _learn_with_snapshots(model, total):
    snaps, train = [], model.train

    def spy():
        before = model.policy.flat_param.detach().clone()
        rec = train()
        snaps.append((before, model.policy.flat_param.detach().clone()))
        return rec
    model.train = spy
    model.learn(total)
    return snaps


def test_schedules_follow_progress_remaining_and_a_zero_learning_rate_freezes_the_policy(cpu_rollout, tmp_path):
    """4 iterations of 4 envs x 8 steps: progress_remaining before the updates is .75, .5, .25, 0 (SB3's rule, evaluated after the rollout)."""
    model = amd.PPO(_StandInEnv(4), n_steps=8, batch_size=16, n_epochs=2, bootstrap_truncated=False, seed=5,
                    learning_rate=lambda p: 2e-4 if p > 0.4 else 0.0, clip_range=lambda p: 0.2 if p > 0.4 else 0.1)
    assert model.learning_rate == 2e-4 and model.clip_range == 0.2          # progress 1 outside learn
    snaps = _learn_with_snapshots(model, 4 * 32)
    assert [r["learning_rate"] for r in model.log] == [2e-4, 2e-4, 0.0, 0.0]
    assert [r["clip_range"] for r in model.log] == [0.2, 0.2, 0.1, 0.1]
    for before, after in snaps[:2]:
        assert not torch.equal(before, after)
    for before, after in snaps[2:]:
        assert torch.equal(before, after)                                    # bit-identical across the updates of the second half
    assert [r["n_updates"] for r in model.log] == [4, 8, 12, 16]            # (Adam steps are applied, with a zero step size)
    for r in model.log:
        assert all(isinstance(v, (int, float)) and math.isfinite(v) for v in r.values())
        assert {"approx_kl", "explained_variance", "std", "n_updates", "learning_rate", "clip_range", "kl_early_stop"} <= set(r)
        assert r["kl_early_stop"] == 0 and r["std"] == pytest.approx(float(model.policy.log_std.detach().exp().mean()), rel=1e-3)
    # a train() outside learn is at progress 1 again
    model.train()
    assert model.learning_rate == 2e-4 and model.clip_range == 0.2
    # checkpoint: the current numbers, target_kl and n_updates; no schedule inside; load restores n_updates
    path = model.save(str(tmp_path / "m"))
    import json
    import zipfile
    data = json.loads(zipfile.ZipFile(path).read("data"))
    assert data["learning_rate"] == 2e-4 and data["clip_range"] == 0.2 and data["target_kl"] is None and data["n_updates"] == model.n_updates == 20
    fresh = amd.PPO(_StandInEnv(4), n_steps=8, batch_size=16, n_epochs=2, bootstrap_truncated=False, target_kl=0.02)
    fresh.load(path)
    assert fresh.n_updates == 20 and fresh.target_kl == 0.02


def test_learn_with_target_kl_on_the_host_path_counts_only_applied_steps(cpu_rollout):
    model = amd.PPO(_StandInEnv(4), n_steps=8, batch_size=16, n_epochs=4, bootstrap_truncated=False, seed=5, learning_rate=3e-2, target_kl=1e-4)
    model.learn(2 * 32)
    assert all(r["kl_early_stop"] == 1 for r in model.log) and model.log[-1]["n_updates"] < 2 * 8
    assert all(math.isfinite(v) for r in model.log for v in r.values()) and model.log[0]["n_updates"] <= model.log[1]["n_updates"]
