"""PPO on the 1- and 2-link arm vehicles (obs_dim 25 / 27, act_dim 5 / 6): the training kernels at those dimensions against their torch
restatements (sampling, fused loss, both forward kernels, the fused minibatch step), the one-launch closed loop for every fp32 arm config
outside the lane-team kernel's (1- / 2-link arms, 2..4 waypoints, general joint axes: the env part replays bit for bit through amenv_step's
lane kernel, the caller's row widths, the policy part against the fp32 modules), the PID warm start on the shorter arms, and PPO end to end."""
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.ppo import PPO, ActorCritic, MinibatchStep, gaussian_act

pytestmark = pytest.mark.gpu


def _bounds(A, dev):
    return torch.tensor([0.0] + [-1.0] * (A - 1), device=dev), torch.tensor([2.0] + [1.0] * (A - 1), device=dev)


@pytest.mark.parametrize("A", [5, 6])
def test_gaussian_act_at_5_and_6_actions(A):
    """Moments / independence / tails of the noise, log-prob = the diagonal Gaussian's, clip = the box; and the prefix identity: for the same
    (seed, env id, draw) and the same mean / log_std prefixes the first A raw and clipped entries equal the 7-entry kernel's bit for bit."""
    n, dev = 200000, "cuda"
    torch.manual_seed(A)
    mean7 = torch.randn(n, 7, device=dev)
    ls7 = torch.linspace(-1.0, 0.3, 7, device=dev)
    mean, log_std = mean7[:, :A].contiguous(), ls7[:A].contiguous()
    low, high = _bounds(A, dev)
    raw, clipped, logp = torch.zeros(n, A, device=dev), torch.zeros(n, A, device=dev), torch.zeros(n, device=dev)
    gaussian_act(mean, log_std, low, high, raw, clipped, logp, seed=7, draw=3)
    z = ((raw - mean) * torch.exp(-log_std)).double()
    assert float(z.mean(0).abs().max()) < 0.01 and float((z.var(0) - 1).abs().max()) < 0.02
    assert float(((z ** 4).mean(0) - 3).abs().max()) < 0.1
    assert float((torch.corrcoef(z.T) - torch.eye(A, device=dev, dtype=torch.float64)).abs().max()) < 0.01
    assert 4.0 < float(z.abs().max()) < 6.5
    ref = torch.distributions.Normal(mean, log_std.exp()).log_prob(raw).sum(-1)
    assert float((logp - ref).abs().max()) < 2e-4
    assert torch.equal(clipped, torch.minimum(torch.maximum(raw, low), high))
    low7, high7 = _bounds(7, dev)
    raw7, clipped7, logp7 = torch.zeros(n, 7, device=dev), torch.zeros(n, 7, device=dev), torch.zeros(n, device=dev)
    gaussian_act(mean7, ls7, low7, high7, raw7, clipped7, logp7, seed=7, draw=3)
    assert torch.equal(raw, raw7[:, :A]) and torch.equal(clipped, clipped7[:, :A])
    h = n // 2
    ra, ca, la = torch.zeros(h, A, device=dev), torch.zeros(h, A, device=dev), torch.zeros(h, device=dev)
    gaussian_act(mean[h:].contiguous(), log_std, low, high, ra, ca, la, seed=7, draw=3, env_id_offset=h)
    assert torch.equal(ra, raw[h:]) and torch.equal(la, logp[h:])


@pytest.mark.parametrize("A,normalize", [(5, True), (6, True), (6, False)])
def test_fused_ppo_loss_at_5_and_6_actions(A, normalize):
    """amenv_ppo_loss_grad at act_dim 5 / 6 against SB3's loss in fp64 through autograd (the gates of the 4 / 7 test)."""
    torch.manual_seed(A)
    n, D, dev = 10007, 23 + 2 * (A - 4), "cuda"
    pol = ActorCritic(D, A).to(dev).flatten_()
    with torch.no_grad():
        pol.log_std.data.copy_(torch.linspace(-0.7, 0.2, A))
    obs = torch.randn(n, D, device=dev)
    with torch.no_grad():
        mean = pol.actor(obs)
    actions = (mean + torch.randn(n, A, device=dev) * pol.log_std.detach().exp() * 1.5).contiguous()
    old_logp = (pol.evaluate_actions(obs, actions)[1].detach() + 0.3 * torch.randn(n, device=dev)).contiguous()
    adv = (torch.randn(n, device=dev) * 3 + 0.5).contiguous()
    ret = (torch.randn(n, device=dev) * 10).contiguous()
    leaf = pol.flat_param.requires_grad_(True)
    opt = torch.optim.SGD([leaf], lr=0.0)
    fused = MinibatchStep(pol, opt, normalize_advantage=normalize, use_graph=False, fused_loss=True, fused_mlp=False)
    fused._forward_backward(obs, actions, old_logp, adv, ret)
    g_fused, s_fused = pol.flat_grad.clone(), fused.stats.clone()
    pol64 = ActorCritic(D, A).to(dev).double()
    pol64.load_state_dict({k: v.double() for k, v in pol.state_dict().items()})
    a64 = adv.double()
    if normalize:
        a64 = (a64 - a64.mean()) / (a64.std() + 1e-8)
    values, logp, ent = pol64.evaluate_actions(obs.double(), actions.double())
    ratio = torch.exp(logp - old_logp.double())
    pl = -torch.min(a64 * ratio, a64 * ratio.clamp(0.8, 1.2)).mean()
    vl = ((ret.double() - values) ** 2).mean()
    el = -ent.mean()
    grads = torch.autograd.grad(pl + 5e-4 * el + 0.5 * vl, list(pol64.parameters()))
    g_ref = torch.cat([g.reshape(-1) for g in grads])
    scale = g_ref.abs().max()
    assert float((g_fused.double() - g_ref).abs().max() / scale) < 2e-5
    ref_stats = torch.stack([pl, vl, el, ((ratio - 1).abs() > 0.2).double().mean()])
    assert float(((s_fused[:4].double() - ref_stats).abs() / ref_stats.abs().clamp(min=1e-3)).max()) < 1e-4
    assert 0.05 < float(ref_stats[3]) < 0.95


@pytest.mark.parametrize("D,A", [(25, 5), (27, 6)])
@pytest.mark.parametrize("n", [1, 1000, 32768])
def test_fused_forward_kernels_at_the_shorter_arms(D, A, n):
    """amenv_policy_forward (VALU) and amenv_policy_forward_mfma, both at every n, against the fp32 torch modules (2e-5 of the scale)."""
    import ctypes as C
    torch.manual_seed(D * 100 + A)
    pol = ActorCritic(D, A).to("cuda").flatten_()
    with torch.no_grad():
        pol.flat_param.mul_(1.7)
        pol.action_net.weight.mul_(30.0)
    obs = torch.randn(n, D, device="cuda") * 1.5
    with torch.no_grad():
        assert pol.fused_ok(obs)
        ref_mean = pol.action_net(pol.mlp_extractor.policy_net(obs))
        ref_value = pol.value_net(pol.mlp_extractor.value_net(obs)).squeeze(-1)
        mean, value = pol.actor_critic(obs)
    assert mean.shape == (n, A) and value.shape == (n,)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ws = torch.empty(L.load().amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp = pol.flat_param.detach()
    got = {}
    for form in ("valu", "mfma"):
        m, v = torch.empty(n, A, device="cuda"), torch.empty(n, device="cuda")
        if form == "valu":
            rc = L.load().amenv_policy_forward(p(fp), D, A, p(obs), n, p(m), p(v), stream)
        else:
            rc = L.load().amenv_policy_forward_mfma(p(fp), D, A, p(obs), n, p(m), p(v), p(ws), stream)
        assert rc == 0, form
        torch.cuda.synchronize()
        assert float((m - ref_mean).abs().max()) < 2e-5 * max(1.0, float(ref_mean.abs().max())), form
        assert float((v - ref_value).abs().max()) < 2e-5 * max(1.0, float(ref_value.abs().max())), form
        got[form] = (m, v)
    m, v = got["mfma" if n >= pol.MFMA_FORWARD_ROWS else "valu"]          # the inference path takes the kernel its batch size selects
    assert torch.equal(mean, m) and torch.equal(value, v)


@pytest.mark.parametrize("D,A,n", [(25, 5, 8192), (27, 6, 20011), (25, 5, 31)])   # 20011, 31: ragged
def test_fused_mlp_step_at_the_shorter_arms(D, A, n):
    """amenv_ppo_mlp_step at (25,5) / (27,6) against autograd on the fp32 modules: every entry within 2e-5 of the largest, every parameter
    block within 1e-4 of its own largest, the four scalars equal."""
    torch.manual_seed(3)
    pol = ActorCritic(D, A).cuda().flatten_()
    with torch.no_grad():
        pol.log_std.data.copy_(torch.linspace(-0.7, 0.2, A))
        pol.action_net.weight.mul_(20.0)
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-3)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(n, D, device="cuda", generator=g) * 0.7
    with torch.no_grad():
        mean = pol.action_net(pol.mlp_extractor.policy_net(obs))
    actions = mean + torch.exp(pol.log_std.detach()) * torch.randn(n, A, device="cuda", generator=g)
    with torch.no_grad():
        _, logp, _ = pol.evaluate_actions(obs, actions)
    old_logp = logp + 0.15 * torch.randn(n, device="cuda", generator=g)
    adv = torch.randn(n, device="cuda", generator=g) * 3.0 + 0.5
    ret = torch.randn(n, device="cuda", generator=g) * 2.0
    outs = []
    for fused in (False, True):
        step = MinibatchStep(pol, opt, clip_range=0.2, ent_coef=5e-4, vf_coef=0.5, use_graph=False, fused_loss=False, fused_mlp=fused)
        assert step.fused_mlp == fused
        pol.flat_grad.zero_()
        step._forward_backward(obs, actions, old_logp, adv, ret)
        torch.cuda.synchronize()
        outs.append((pol.flat_grad.clone(), step.stats[:4].clone()))
    (g0, s0), (g1, s1) = outs
    scale = float(g0.abs().max())
    assert scale > 0 and float((g0 - g1).abs().max()) < 2e-5 * scale, (float((g0 - g1).abs().max()), scale)
    off = 0
    for p_ in pol.parameters():
        k = p_.numel()
        blk = float(g0[off:off + k].abs().max())
        assert float((g0[off:off + k] - g1[off:off + k]).abs().max()) < 1e-4 * max(blk, 1e-3 * scale), (off, k)
        off += k
    assert torch.allclose(s0, s1, rtol=2e-4, atol=1e-6), (s0, s1)
    if n > 1000:
        assert 0.02 < float(s1[3]) < 0.9


def _arm_env(n, nj, K, axes, **kw):
    cfg = L.default_config("hexa_arm", n, n_joints=nj)
    cfg.seed = 4
    cfg.task.max_episode_steps = 60
    if K > 1:
        cfg.task.num_waypoints = K
        for k in range(1, K + 1):
            cfg.task.traj_sin[k - 1] = math.sin(2.0 * (k / K) * math.pi)
            cfg.task.traj_cos[k - 1] = math.cos((k / K) * 2.0 * math.pi)
    if axes is not None:
        for k, ax in enumerate(axes):
            for j in range(3):
                cfg.vehicle.joint_axis[3 * k + j] = 1.0 if j == "xyz".index(ax) else 0.0
    if "kernel" in kw:
        cfg.step_kernel = L.KERNELS[kw["kernel"]]
    return amd.GpuWaypointEnv(n, config=cfg)


@pytest.mark.parametrize("nj,K,axes,n", [(1, 1, None, 300), (2, 1, None, 300), (1, 1, None, 20000), (2, 1, None, 20000),
                                         (3, 2, None, 3000), (3, 4, None, 3000), (3, 1, "zyx", 3000)])
def test_arm_closed_loop_one_launch(nj, K, axes, n):
    """amenv_rollout_policy on the arm configs outside the lane-team kernel's: rows of the caller's widths (23 + 2 nj / 4 + nj); the env part
    replays bit for bit through amenv_step on a lane-kernel handle (obs, rewards, dones, info, terminal rows, final state, Monitor totals); the
    policy part against the fp32 modules on the recorded rows (bf16 tolerance); the noise statistically, log-probs over the 4 + nj entries;
    the same call from the same state gives the same outputs."""
    T = 96
    env = _arm_env(n, nj, K, axes)
    ref = _arm_env(n, nj, K, axes, kernel="lane")
    od, A = env.obs_dim, env.act_dim
    assert (od, A) == (23 + 2 * nj, 4 + nj) and "step_kernel<" in ref.kernel_name
    torch.manual_seed(5 + nj)
    pol = ActorCritic(od, A).cuda().flatten_()
    with torch.no_grad():
        pol.log_std.data.fill_(-1.2)
        pol.action_net.weight.mul_(30.0)
    o0 = env.reset().clone(); ref.reset()
    dev = env.device
    mk = lambda: dict(obs=torch.zeros(T + 1, n, od, device=dev), actions=torch.zeros(T, n, A, device=dev), logp=torch.zeros(T, n, device=dev),  # noqa: E731
                      values=torch.zeros(T, n, device=dev), rewards=torch.zeros(T, n, device=dev), dones=torch.zeros(T, n, dtype=torch.uint8, device=dev))
    b = mk()
    info = torch.zeros(T, n, dtype=torch.int32, device=dev); tobs = torch.full((T, n, od), float("nan"), device=dev)
    env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, info_bits=info, terminal_obs=tobs, **b)
    torch.cuda.synchronize()
    assert float((b["obs"][0] - o0).abs().max()) < 1e-6
    lo, hi = pol.action_low, pol.action_high
    for t in range(T):
        o, r, d, i = ref.step(torch.max(torch.min(b["actions"][t], hi), lo))
        assert torch.equal(o, b["obs"][t + 1]) and torch.equal(r, b["rewards"][t]) and torch.equal(d, b["dones"][t]) and torch.equal(i, info[t]), t
        dn = d.bool()
        if bool(dn.any()):
            assert torch.equal(ref.terminal_obs[dn], tobs[t][dn]), t
    f1, i1 = env.get_state(); f2, i2 = ref.get_state()
    assert torch.equal(f1, f2) and torch.equal(i1, i2)
    s1, s2 = env.stats(), ref.stats()
    assert s1 == s2 and s1["episodes"] == int(b["dones"].sum()) > n // 2, (s1, s2)
    assert bool(torch.isnan(tobs[~b["dones"].bool()]).all())
    with torch.no_grad():
        flat = b["obs"][:T].reshape(T * n, od)
        mean32 = pol.action_net(pol.mlp_extractor.policy_net(flat)); v32 = pol.value_net(pol.mlp_extractor.value_net(flat)).reshape(-1)
    std = torch.exp(pol.log_std.detach())
    assert float((b["values"].reshape(-1) - v32).abs().max()) < 3e-2 * max(1.0, float(v32.abs().max()))
    z = (b["actions"].reshape(T * n, A) - mean32) / std
    assert abs(float(z.mean())) < 0.02 and abs(float(z.var()) - 1.0) < 0.03 and float(z.abs().max()) < 6.5
    assert float((torch.corrcoef(z[:50000].T) - torch.eye(A, device=dev)).abs().max()) < 0.03
    lp32 = (-0.5 * z * z - pol.log_std.detach() - 0.9189385332).sum(1)
    assert float((b["logp"].reshape(-1) - lp32).abs().max()) < 0.5 and float((b["logp"].reshape(-1) - lp32).abs().mean()) < 0.05
    env2 = _arm_env(n, nj, K, axes); env2.reset()
    b2 = mk()
    info2 = torch.zeros_like(info); tobs2 = torch.full_like(tobs, float("nan"))
    env2.rollout_policy(pol.flat_param, T, seed=77, draw0=5, info_bits=info2, terminal_obs=tobs2, **b2)
    assert all(torch.equal(b2[k], b[k]) for k in b) and torch.equal(info2, info) and torch.equal(tobs2.nan_to_num(7.0), tobs.nan_to_num(7.0))
    env.close(); ref.close(); env2.close()


def test_pid_policy_on_a_two_link_arm():
    """amenv_pid_policy in tool mode reads the tool offset from the last three columns: on the 27-wide rows of a 2-link arm its actions are the
    first 6 entries of the 7-action PID on the same rows laid out 29 wide (tool columns at 26..28), bit for bit; clone_pid_policy runs on a
    1-link arm."""
    n = 512
    env = amd.GpuWaypointEnv(n, vehicle="hexa_arm", n_joints=2, seed=2)
    obs = env.reset()
    pid6 = amd.PidWaypointPolicy.for_env(env)
    assert pid6.tool_mode and pid6.act_dim == 6
    pid7 = amd.PidWaypointPolicy.for_env(env)
    pid7.act_dim = 7
    done = None
    for _ in range(40):
        o29 = torch.zeros(n, 29, device=obs.device)
        o29[:, :22] = obs[:, :22]; o29[:, 23:25] = obs[:, 22:24]; o29[:, 26:29] = obs[:, 24:27]
        a6 = pid6.predict(obs, done); a7 = pid7.predict(o29, done)
        assert a6.shape == (n, 6) and torch.equal(a6, a7[:, :6]) and bool((a6[:, 4:] == 0).all())
        obs, _, done, _ = env.step(a6)
    env.close()
    env1 = amd.GpuWaypointEnv(256, vehicle="hexa_arm", n_joints=1, seed=2)
    pol = ActorCritic(env1.obs_dim, env1.act_dim).cuda()
    amd.clone_pid_policy(env1, pol, steps=100, epochs=20, dagger_rounds=1)
    assert float(pol.log_std.data.max()) == -1.0 and all(bool(torch.isfinite(p).all()) for p in pol.parameters())
    env1.close()


@pytest.mark.parametrize("nj", [1, 2])
@pytest.mark.parametrize("fused_rollout", [False, True])
def test_ppo_on_the_shorter_arms(nj, fused_rollout):
    """PPO(env).learn on a 1- / 2-link arm, step by step and one-launch: the fused minibatch step is selected, the parameters move, every
    logged value is finite."""
    env = amd.GpuWaypointEnv(1024, vehicle="hexa_arm", n_joints=nj, seed=3, max_episode_steps=100)
    algo = PPO(env, n_steps=32, batch_size=8192, n_epochs=2, seed=1, fused_rollout=fused_rollout)
    with torch.no_grad():
        assert algo._step.fused_mlp and algo.policy.fused_ok(torch.zeros(4, env.obs_dim, device=env.device))
    p0 = algo.policy.flat_param.detach().clone()
    algo.learn(3 * 32 * 1024)
    assert len(algo.log) == 3
    assert all(math.isfinite(float(v)) for rec in algo.log for v in rec.values())
    assert float((algo.policy.flat_param.detach() - p0).abs().max()) > 0
    assert algo.buffer.actions.shape[-1] == 4 + nj and bool(torch.isfinite(algo.buffer.obs).all())
    env.close()
