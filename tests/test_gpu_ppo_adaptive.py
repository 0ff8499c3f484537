"""KL-adaptive learning rate on the GPU: amenv_ppo_adam_step_adapt against the plain kernel given the rate the rule yields
(bit-identical, every case of the CPU table, the stop, every refusal), a sequence of minibatch steps whose every rate is the rule's bit for
bit, the fused path against the torch path, and `PPO.learn` end to end with save / load and with target_kl."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.ppo import ActorCritic, KlAdaptiveLr, MinibatchStep, PPO
from tests.test_ppo_adaptive_cpu import RULE_TABLE

pytestmark = pytest.mark.gpu
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
KL_LAST, STOP, APPLIED = L.PpoCtl.kl_last.offset // 4, L.PpoCtl.stop.offset // 4, L.PpoCtl.applied.offset // 4
POLICY_29_7 = ActorCritic(29, 7).num_parameters()


def _armed(kl, stop=0):
    """A control block as the loss of a minibatch leaves it: kl_last written into the block's tensor from here."""
    t = torch.zeros(C.sizeof(L.PpoCtl) // 4, dtype=torch.int32, device="cuda")
    assert L.load().amenv_ppo_ctl_arm(ptr(t), 0.0, None) == 0
    t.view(torch.float32)[KL_LAST] = float(np.float32(kl))
    t[STOP] = stop
    return t


def _adam_buffers(n, lr, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    prm, grad = torch.randn(n, device="cuda", generator=g), torch.randn(n + 4, device="cuda", generator=g)[:n] * 0.3   # (16-byte aligned base)
    m, v = torch.randn(n, device="cuda", generator=g) * 0.1, torch.rand(n, device="cuda", generator=g) * 0.01
    stp, gn, ticket = torch.full((), 3.0, device="cuda"), torch.full((1,), -1.0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    hyper = torch.tensor([lr, 0.9, 0.999, 1e-5, 0.5, 1.0], device="cuda")
    return [prm, grad, m, v, stp, hyper, gn, ticket]


def _call(fn, b, n, ctl, *tail):
    prm, grad, m, v, stp, hyper, gn, ticket = b
    return fn(ptr(prm), ptr(grad), ptr(m), ptr(v), ptr(stp), n, ptr(hyper), ptr(gn), ptr(ticket), ptr(ctl), *tail, None)


@pytest.mark.parametrize("n", [4099, POLICY_29_7])     # 4099: five workgroups, a ragged last one, n % 4 != 0; the (29, 7) policy's count
def test_one_adam_step_equals_the_plain_kernel_at_the_rules_rate(n):
    lib, rule = L.load(), KlAdaptiveLr()
    rs = rule.struct()
    for lr, kl, want in RULE_TABLE:
        a, b = _adam_buffers(n, lr), _adam_buffers(n, lr)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        new = rule.step(lr, kl)
        assert float(new) == want
        b[5][0] = float(new)
        ctl_a, ctl_b = _armed(kl), _armed(kl)
        assert _call(lib.amenv_ppo_adam_step_adapt, a, n, ctl_a, C.byref(rs)) == 0
        assert _call(lib.amenv_ppo_adam_step_ctl, b, n, ctl_b) == 0
        for name, x, y in zip(("params", "grad", "exp_avg", "exp_avg_sq", "step", "hyper6", "grad_norm", "ticket"), a, b):
            assert torch.equal(x, y), (name, lr, kl)
        h = a[5].cpu().numpy()
        assert h[0] == np.float32(want) and h[1:].tolist() == np.array([0.9, 0.999, 1e-5, 0.5, 1.0], dtype=np.float32).tolist()
        assert float(a[4]) == 4.0 and int(a[7]) == 0 and int(ctl_a[APPLIED]) == 1 and torch.equal(ctl_a, ctl_b)


def test_stop_and_invalid_arguments_change_nothing():
    lib, n = L.load(), 4099
    rs = KlAdaptiveLr().struct()
    # the gate is shut: a kl that would lower the rate, and nothing moves -- hyper6, the step counter and the ticket included
    a, ref = _adam_buffers(n, 2e-4), _adam_buffers(n, 2e-4)
    ctl = _armed(0.05, stop=1)
    before = ctl.clone()
    assert _call(lib.amenv_ppo_adam_step_adapt, a, n, ctl, C.byref(rs)) == 0
    assert all(torch.equal(x, y) for x, y in zip(a, ref)) and torch.equal(ctl, before)
    # refusals: -1, nothing enqueued
    ctl = _armed(0.05)
    before = ctl.clone()

    def bad(**kw):
        r = KlAdaptiveLr().struct()
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    rules = [bad(struct_size=20), bad(struct_size=0), bad(desired_kl=0.0), bad(desired_kl=-1.0), bad(desired_kl=float("nan")), bad(desired_kl=float("inf")),
             bad(band=0.5), bad(band=float("nan")), bad(factor=1.0), bad(factor=float("inf")), bad(lr_min=0.0), bad(lr_min=float("nan")),
             bad(lr_min=2e-2), bad(lr_max=float("inf")), bad(lr_max=float("nan"))]
    for r in rules:
        assert _call(lib.amenv_ppo_adam_step_adapt, a, n, ctl, C.byref(r)) == -1, [getattr(r, f[0]) for f in r._fields_]
    assert _call(lib.amenv_ppo_adam_step_adapt, a, n, None, C.byref(rs)) == -1                     # ctl must be given
    assert _call(lib.amenv_ppo_adam_step_adapt, a, n, ctl, None) == -1                             # and the rule
    for k in (0, 1, 2, 3, 4, 5, 7):                                                                # a NULL buffer (grad_norm_out may be NULL)
        c = list(a)
        c[k] = None
        assert _call(lib.amenv_ppo_adam_step_adapt, c, n, ctl, C.byref(rs)) == -1, k
    assert _call(lib.amenv_ppo_adam_step_adapt, a, 0, ctl, C.byref(rs)) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, ref)) and torch.equal(ctl, before)


# ---- a sequence of minibatch steps ------------------------------------------------------------------------------------------------
LR0 = 3e-3          # the data and the rate of tests/test_gpu_ppo_controls.py's gate tests: approx_kl grows from minibatch to minibatch


def _rollout_problem(D, A, n, seed=1):
    """Rollout-shaped data (as the gate tests build it): the old log-probs are the policy's own, so approx_kl starts at 0 and grows."""
    torch.manual_seed(3)
    pol = ActorCritic(D, A).cuda().flatten_()
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randn(n, D, device="cuda", generator=g) * 0.7
    with torch.no_grad():
        actions = (pol.actor(obs) + torch.randn(n, A, device="cuda", generator=g)).contiguous()
        _, old_logp, _ = pol.evaluate_actions(obs, actions)
    adv = torch.randn(n, device="cuda", generator=g) * 3.0 + 0.5
    ret = torch.randn(n, device="cuda", generator=g) * 2.0
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=LR0, eps=1e-5, capturable=True)
    pol.flat_param.grad = pol.flat_grad
    return pol, opt, (obs, actions, old_logp.contiguous(), adv, ret)


def _perms(n, mb, epochs, seed=11):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [p[s:s + mb] for p in (torch.randperm(n, device="cuda", generator=gen) for _ in range(epochs)) for s in range(0, n, mb)]


def _trace(D, A, mb, fused=True, **kw):
    """12 minibatch steps; per step (approx_kl, learning rate after it).  Synchronises after every step: this is a test."""
    pol, opt, data = _rollout_problem(D, A, 4 * mb)
    step = MinibatchStep(pol, opt, use_graph=False, fused_mlp=fused, **kw)
    assert step.fused_mlp == fused and step.fused_adam == fused
    out = []
    for idx in _perms(4 * mb, mb, 3):
        if fused:
            step.indexed(*data, idx)
        else:
            step(*[t[idx].contiguous() for t in data])
        lr = float(step._adam_hyper[0]) if step.device_rule else float(np.float32(opt.param_groups[0]["lr"]))
        out.append((float(step.kl), lr))
    return out, step, pol, opt


def _desired_kl(kls):
    """From the unadapted trace: the geometric mean of the second and the last minibatch's approx_kl.  Where the last is >= 8 x the
    second (4 x would do: the margin is 1.4 on either side), the second is below desired / 2 (a raise) and the trace ends above 2 desired (a lowering: once the rate has been raised
    the update moves no slower than the unadapted one)."""
    assert kls[1] > 0 and kls[-1] >= 8 * kls[1], f"test data: approx_kl does not grow 8-fold over the 12 steps: {kls}"
    return math.sqrt(kls[1] * kls[-1])


def _category(rule, kl):
    kl = np.float32(kl)
    return -1 if kl > rule.band * rule.desired_kl else 1 if (kl > 0 and kl < rule.desired_kl / rule.band) else 0


@pytest.mark.parametrize("D,A", [(20, 4), (29, 7)])
def test_every_learning_rate_of_a_sequence_is_the_rules(D, A):
    mb = 1000
    plain, _, _, _ = _trace(D, A, mb)
    kls = [k for k, _ in plain]
    assert all(lr == float(np.float32(LR0)) for _, lr in plain)
    rule = KlAdaptiveLr(desired_kl=_desired_kl(kls))
    got, step, pol, opt = _trace(D, A, mb, adaptive_lr=rule)
    assert step.device_rule and not step.device_gate
    print(f"unadapted approx_kl {['%.3g' % k for k in kls]}; desired_kl {float(rule.desired_kl):.4g}")
    print("adapted (kl, lr): " + " ".join(f"({k:.3g}, {lr:.4g})" for k, lr in got))
    prev, moves = np.float32(LR0), []
    for j, (kl, lr) in enumerate(got):
        want = rule.step(prev, kl)
        assert np.float32(lr) == want, (j, kl, float(prev), lr, float(want))
        moves.append(int(np.sign(float(want) - float(prev))))
        prev = want
    assert 1 in moves and -1 in moves, moves                                       # the condition on the input: both directions occur
    # the host has not been told yet: the update's one transfer brings the rate back
    assert opt.param_groups[0]["lr"] == LR0
    rec, _ = step.readout(torch.zeros(6, device="cuda"), 1)
    assert opt.param_groups[0]["lr"] == float(prev) and math.isfinite(rec["approx_kl"])
    # and the next step does not upload the host's copy over it
    step.indexed(*_rollout_problem(D, A, 4 * mb)[2], _perms(4 * mb, mb, 1)[0])
    assert np.float32(float(step._adam_hyper[0])) == rule.step(prev, float(step.kl))


def test_fused_and_torch_paths_take_the_same_decisions():
    """The device rule against the host rule on the torch path (fused loss + torch modules + torch Adam), same data and rule: the same
    decision at every minibatch whose approx_kl is not within 1 % of a threshold.  A minibatch inside that margin may go either way, and
    the two runs are not comparable after one whose rates then differ.  The rule's third threshold is kl > 0, and the first minibatch
    sits on it: the old log-probs are the policy's own, each sample's (r - 1) - log r carries one rounding of r ~ 1 (6e-8), and the mean
    comes out as +-1e-8 on either path -- |kl| <= 1e-6 counts as inside the margin.  So that this does not end the comparison at its first
    step the run starts AT lr_max: a raise there is clamped, the rates stay equal, and the decisions that follow are comparable."""
    D, A, mb = 20, 4, 1000
    plain, _, _, _ = _trace(D, A, mb)
    rule = KlAdaptiveLr(desired_kl=_desired_kl([k for k, _ in plain]), lr_max=LR0)
    hi, lo = float(rule.band * rule.desired_kl), float(rule.desired_kl / rule.band)
    fused, sf, _, _ = _trace(D, A, mb, adaptive_lr=rule)
    torch_, st, _, opt_t = _trace(D, A, mb, fused=False, adaptive_lr=rule)
    assert sf.device_rule and not st.device_rule and st.fused_loss
    prev_f = prev_t = np.float32(LR0)
    compared = 0
    for j, ((kf, lf), (kt, lt)) in enumerate(zip(fused, torch_)):
        assert np.float32(lf) == rule.step(prev_f, kf) and np.float32(lt) == rule.step(prev_t, kt), j     # each path follows the rule on its own kl
        near = any(abs(k - t) <= 0.01 * t for k in (kf, kt) for t in (hi, lo)) or any(abs(k) <= 1e-6 for k in (kf, kt))
        cf, ct = _category(rule, kf), _category(rule, kt)
        print(f"minibatch {j}: fused kl {kf:.5g} -> {cf:+d} lr {lf:.5g} | torch kl {kt:.5g} -> {ct:+d} lr {lt:.5g}{'  (within 1 % of a threshold)' if near else ''}")
        if near and cf != ct and lf != lt:
            break
        assert cf == ct or near, (j, kf, kt)
        assert lf == lt, (j, lf, lt)
        prev_f, prev_t = np.float32(lf), np.float32(lt)
        compared += 1
    assert compared >= 6 and np.float32(fused[-1][1]) < np.float32(LR0), (compared, fused[-1])      # and the rate was lowered on the way


def test_the_rate_does_not_move_after_the_stop():
    """adaptive_lr with target_kl on the device: the minibatch that trips the gate has its loss evaluated and neither its optimiser step
    nor its rule; afterwards nothing moves."""
    D, A, mb = 29, 7, 1000
    plain, _, _, _ = _trace(D, A, mb)
    rule = KlAdaptiveLr(desired_kl=_desired_kl([k for k, _ in plain]))
    free, _, _, _ = _trace(D, A, mb, adaptive_lr=rule)
    j = next((i for i in range(3, 12) if free[i][0] > 1.2 * max(k for k, _ in free[:i])), None)   # the first step (past the third) that tops the earlier ones
    assert j is not None, f"test data: no minibatch tops the earlier ones by 1.2x: {free}"
    limit = math.sqrt(free[j][0] * max(k for k, _ in free[:j]))
    got, step, pol, opt = _trace(D, A, mb, adaptive_lr=rule, target_kl=limit / 1.5)
    assert step.device_rule and step.device_gate
    c = L.PpoCtl.from_buffer_copy(step._ctl.cpu().numpy().tobytes())
    assert (c.evaluated, c.applied, c.stop) == (j + 1, j, 1)
    assert got[:j] == free[:j]                                                                # the same steps up to the stop
    assert got[j][0] == free[j][0] and all(x == (got[j][0], got[j - 1][1]) for x in got[j:])   # kl_last stays, the rate is step j - 1's
    assert float(opt.state[opt.param_groups[0]["params"][0]]["step"]) == j


# ---- the whole loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target_kl", [None, 0.01])
def test_learn_with_adaptive_lr(target_kl, tmp_path):
    rule = KlAdaptiveLr()
    env = amd.GpuWaypointEnv(256, seed=2)
    algo = PPO(env, n_steps=64, batch_size=4096, n_epochs=4, seed=1, adaptive_lr=rule, target_kl=target_kl, fused_rollout=True)
    assert algo._step.device_rule and not algo._step.use_graph and algo._step.device_gate == (target_kl is not None)
    lrs = []
    algo.learn(3 * 64 * 256, log_fn=lambda rec: lrs.append((rec["learning_rate"], algo.optimizer.param_groups[0]["lr"], float(algo._step._adam_hyper[0]))))
    assert len(algo.log) == 3
    for rec, (logged, group, device) in zip(algo.log, lrs):
        assert all(isinstance(v, (int, float)) and math.isfinite(v) for v in rec.values()), rec
        assert float(rule.lr_min) <= logged <= float(rule.lr_max) and logged == group == device, (logged, group, device)
        assert rec["kl_early_stop"] in (0, 1) and (target_kl is not None or rec["kl_early_stop"] == 0)
    print("learning rates", [x[0] for x in lrs], "approx_kl", [r["approx_kl"] for r in algo.log], "stops", [r["kl_early_stop"] for r in algo.log])
    assert any(x[0] != 2e-4 and x[0] != float(np.float32(2e-4)) for x in lrs)                # the rule did move the rate
    path = algo.save(str(tmp_path / "m"))
    env2 = amd.GpuWaypointEnv(256, seed=2)
    fresh = PPO(env2, n_steps=64, batch_size=4096, n_epochs=4, seed=1, adaptive_lr=KlAdaptiveLr(desired_kl=0.05, factor=2.0), target_kl=target_kl,
                fused_rollout=True)
    fresh.load(path)
    assert fresh.learning_rate == algo.learning_rate == lrs[-1][0] and fresh.adaptive_lr == rule and fresh._step.adaptive_lr == rule
    fresh.learn(64 * 256)                                                                     # resumes from that rate: hyper6[0] is uploaded from it
    assert float(rule.lr_min) <= fresh.learning_rate <= float(rule.lr_max) and fresh.learning_rate == float(fresh._step._adam_hyper[0])
    env.close(); env2.close()
