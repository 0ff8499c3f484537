"""KL-adaptive learning rate and clipped value loss on the host paths: the rule bit for bit against float32 values worked out
with exact rational arithmetic, what `KlAdaptiveLr` refuses, the host rule through `MinibatchStep` on CPU tensors, the refusals, and the
clipped value loss of the torch path against fp64 autograd of SB3's formula.  No GPU."""
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd.ppo import ActorCritic, KlAdaptiveLr, MinibatchStep, ppo_update
from tests.test_ppo_controls_cpu import _Dist2, _StandInEnv

H = float.fromhex
# The defaults in float32: desired_kl = 0x1.47ae14p-7 (0.01), so the thresholds are band * desired_kl = 0x1.47ae14p-6 and
# desired_kl / band = 0x1.47ae14p-8 (both exact: band = 2).  Every expected value is the exact quotient / product rounded to nearest even
# to 24 bits, computed with rationals (not with numpy): 2e-4 -> 0x1.a36e2ep-13; / 1.5 -> 0x1.179ecap-13; * 1.5 -> 0x1.3a92a2p-12.
HI, LO = H("0x1.47ae14p-6"), H("0x1.47ae14p-8")
LR, LR_DOWN, LR_UP = H("0x1.a36e2ep-13"), H("0x1.179ecap-13"), H("0x1.3a92a2p-12")
RULE_TABLE = [                                    # (lr, kl, expected), all float32 values
    (2e-4, H("0x1.47ae16p-6"), LR_DOWN),          # one ulp above band * desired_kl: lowered
    (2e-4, HI, LR),                               # on the upper threshold: not above it, unchanged
    (2e-4, H("0x1.47ae12p-8"), LR_UP),            # one ulp below desired_kl / band: raised
    (2e-4, LO, LR),                               # on the lower threshold: unchanged
    (2e-4, 0.01, LR),                             # inside the band
    (2e-4, 0.0, LR),                              # kl = 0 (the first minibatch of an update on the policy's own samples): unchanged
    (2e-4, -1e-9, LR),                            # a rounding-negative estimate: unchanged
    (2e-4, float("nan"), LR),                     # NaN: unchanged
    (1.2e-5, 0.05, H("0x1.4f8b58p-17")),          # 1.2e-5 / 1.5 = 0x1.0c6f7ap-17 (8e-6) < lr_min: clamped to float32(1e-5)
    (8e-3, 1e-3, H("0x1.47ae14p-7")),             # 8e-3 * 1.5 = 0x1.89374cp-7 (1.2e-2) > lr_max: clamped to float32(1e-2)
    (1e-2, 1e-3, H("0x1.47ae14p-7")),             # already at lr_max
    (1e-5, 0.05, H("0x1.4f8b58p-17")),            # already at lr_min
]


def test_the_rule_bit_for_bit():
    rule = KlAdaptiveLr()
    assert (float(rule.desired_kl), float(rule.band), float(rule.factor)) == (H("0x1.47ae14p-7"), 2.0, 1.5)
    for lr, kl, want in RULE_TABLE:
        got = rule.step(lr, kl)
        assert isinstance(got, np.float32) and float(got) == want, (lr, kl, float(got).hex(), want.hex())
    # other numbers: a band of 1 has no dead zone but kl == desired_kl
    tight = KlAdaptiveLr(desired_kl=0.02, factor=2.0, band=1.0, lr_min=1e-4, lr_max=1e-3)
    d = float(np.float32(0.02))
    assert float(tight.step(5e-4, d)) == float(np.float32(5e-4))
    assert float(tight.step(5e-4, np.nextafter(np.float32(d), np.float32(1)))) == float(np.float32(5e-4)) / 2      # (exact: a power of two)
    assert float(tight.step(5e-4, np.nextafter(np.float32(d), np.float32(0)))) == float(np.float32(1e-3))          # 1e-3 = lr_max: clamped onto it
    s = rule.struct()
    assert (s.struct_size, s.desired_kl, s.band, s.factor, s.lr_min, s.lr_max) == (24, rule.desired_kl, 2.0, 1.5, rule.lr_min, rule.lr_max)
    assert KlAdaptiveLr(**rule.state_dict()) == rule and KlAdaptiveLr(desired_kl=0.02) != rule


@pytest.mark.parametrize("kw", [dict(desired_kl=0.0), dict(desired_kl=-0.01), dict(desired_kl=float("nan")), dict(desired_kl=float("inf")),
                                dict(band=0.99), dict(band=float("nan")), dict(factor=1.0), dict(factor=0.5), dict(factor=float("inf")),
                                dict(lr_min=0.0), dict(lr_min=-1e-5), dict(lr_min=2e-2), dict(lr_max=1e-6), dict(lr_max=float("nan")),
                                dict(lr_max=float("inf")), dict(desired_kl="x")])
def test_bad_rules_raise(kw):
    with pytest.raises(amd.AmenvError):
        KlAdaptiveLr(**kw)


def _problem(seed=1, lr=3e-3):
    torch.manual_seed(seed)
    pol = ActorCritic(20, 4).flatten_()
    leaf = pol.flat_param.requires_grad_(True)
    leaf.grad = pol.flat_grad
    g = torch.Generator().manual_seed(0)
    n = 1000
    obs = torch.randn(n, 20, generator=g)
    with torch.no_grad():
        actions = pol.actor(obs) + torch.randn(n, 4, generator=g)
        _, old_logp, _ = pol.evaluate_actions(obs, actions)
        values = pol.critic(obs).clone()
    adv = torch.randn(n, generator=g) * 3.0 + 1.0
    ret = torch.randn(n, generator=g) * 10.0
    return pol, torch.optim.Adam([leaf], lr=lr, eps=1e-5), (obs, actions, old_logp.clone(), adv, ret), values


def test_host_rule_through_minibatch_step():
    """12 minibatch steps on CPU tensors: after each, param_groups[0]['lr'] is step(previous lr, that minibatch's approx_kl); the rate both
    rises (approx_kl starts at 0 < kl < desired / band) and falls (3e-3 x 1.5 x 1.5 drives approx_kl past the band)."""
    pol, opt, data, _ = _problem()
    rule = KlAdaptiveLr(desired_kl=0.004)
    step = MinibatchStep(pol, opt, adaptive_lr=rule)
    assert step.use_graph is False and not step.device_rule
    gen = torch.Generator().manual_seed(7)
    moves = []
    for _ in range(3):
        perm = torch.randperm(1000, generator=gen)
        for s in range(0, 1000, 250):
            idx = perm[s:s + 250]
            prev = opt.param_groups[0]["lr"]
            before = pol.flat_param.detach().clone()
            step(*[t[idx] for t in data])
            kl = float(step.kl)
            want = float(rule.step(prev, kl))
            assert opt.param_groups[0]["lr"] == want, (prev, kl)
            assert not torch.equal(before, pol.flat_param.detach())
            moves.append(np.sign(want - float(np.float32(prev))))
    assert 1.0 in moves and -1.0 in moves, moves
    # through ppo_update, with target_kl as well: after the stop neither the parameters nor the rate move
    pol, opt, data, _ = _problem()
    rec = ppo_update(pol, opt, *data, batch_size=250, n_epochs=3, generator=torch.Generator().manual_seed(7), adaptive_lr=rule, target_kl=0.004)
    assert rec["kl_early_stop"] == 1 and rec["n_updates"] < 12
    assert rule.lr_min <= opt.param_groups[0]["lr"] <= rule.lr_max and opt.param_groups[0]["lr"] == float(np.float32(opt.param_groups[0]["lr"]))


def test_refusals():
    pol = ActorCritic(20, 4).flatten_()
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-4)
    rule = KlAdaptiveLr()
    with pytest.raises(amd.AmenvError, match="use_graph"):
        MinibatchStep(pol, opt, use_graph=True, adaptive_lr=rule)
    with pytest.raises(amd.AmenvError, match="ranks"):
        MinibatchStep(pol, opt, dist=_Dist2(), adaptive_lr=rule)
    with pytest.raises(amd.AmenvError, match="KlAdaptiveLr"):
        MinibatchStep(pol, opt, adaptive_lr=0.01)
    with pytest.raises(amd.AmenvError, match="ranks"):
        amd.PPO(_StandInEnv(2), dist=_Dist2(), adaptive_lr=rule)
    with pytest.raises(amd.AmenvError, match="use_graph"):
        amd.PPO(_StandInEnv(2), use_graph=True, adaptive_lr=rule)
    with pytest.raises(amd.AmenvError, match="two masters"):
        amd.PPO(_StandInEnv(2), learning_rate=lambda p: 2e-4 * p, adaptive_lr=rule)
    with pytest.raises(amd.AmenvError, match="clip_range_vf"):
        MinibatchStep(pol, opt, clip_range_vf=0.0)
    with pytest.raises(amd.AmenvError, match="clip_range_vf"):
        MinibatchStep(pol, opt, clip_range_vf=float("inf"))
    with pytest.raises(amd.AmenvError, match="old_values"):
        MinibatchStep(pol, opt, clip_range_vf=0.2)(*_problem()[2])                  # the clip needs the old values ...
    with pytest.raises(amd.AmenvError, match="old_values"):
        p2, o2, d2, v2 = _problem()
        MinibatchStep(p2, o2)(*d2, v2)                                              # ... and nothing else takes them
    assert MinibatchStep(pol, opt, adaptive_lr=rule).use_graph is False
    model = amd.PPO(_StandInEnv(2), adaptive_lr=rule, clip_range_vf=lambda p: 0.2 * p)
    assert model.learning_rate == 2e-4 and model.clip_range_vf == 0.2 and model._step.adaptive_lr is rule


def test_clipped_value_loss_on_the_torch_path_matches_fp64_autograd():
    """SB3's formula in fp64 autograd against the CPU torch path: value loss and the whole flat gradient; the old values are the critic's
    own plus noise of the clip's size, so a good share of the samples is clipped on either side."""
    c = 0.3
    pol, opt, (obs, actions, old_logp, adv, ret), values = _problem()
    g = torch.Generator().manual_seed(5)
    old_values = values + c * torch.randn(values.shape, generator=g)
    old_logp = old_logp + 0.1 * torch.randn(old_logp.shape, generator=g)
    step = MinibatchStep(pol, opt, clip_range_vf=c)
    step._forward_backward(obs, actions, old_logp, adv, ret, old_values)
    got_grad, got_vl = pol.flat_grad.clone(), float(step.stats[1])

    pol64 = ActorCritic(20, 4).double()
    pol64.load_state_dict({k: v.double() for k, v in pol.state_dict().items()})
    o, a, olp, ad, r, vo = (t.double() for t in (obs, actions, old_logp, adv, ret, old_values))
    ad = (ad - ad.mean()) / (ad.std() + 1e-8)
    v, logp, ent = pol64.evaluate_actions(o, a)
    ratio = (logp - olp).exp()
    pl = -torch.min(ad * ratio, ad * ratio.clamp(0.8, 1.2)).mean()
    v_pred = vo + torch.clamp(v - vo, -c, c)
    vl = ((r - v_pred) ** 2).mean()
    clipped = float(((v - vo).abs() > c).double().mean())
    assert 0.2 < clipped < 0.8, clipped
    grads = torch.autograd.grad(pl + 5e-4 * (-ent.mean()) + 0.5 * vl, list(pol64.parameters()))
    ref = torch.cat([x.reshape(-1) for x in grads])
    scale = float(ref.abs().max())
    err = float((got_grad.double() - ref).abs().max())
    print(f"clipped share {clipped:.3f}; value loss {got_vl:.9g} vs {float(vl.detach()):.9g}; gradient error {err:.3g} of scale {scale:.3g}")
    vl = vl.detach()
    assert abs(got_vl - float(vl)) <= 1e-5 * abs(float(vl))                          # fp32 mean of 1000 squares
    assert err <= 2e-5 * scale                                                       # the bound the fused steps are held to against fp64
    # and the clip does something: the unclipped loss is further away than ten times the tolerance above
    assert abs(float(((r - v.detach()) ** 2).mean()) - float(vl)) > 1e-4 * float(vl)
    assert math.isfinite(got_vl)
