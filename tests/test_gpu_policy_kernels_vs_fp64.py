"""Every hand-written policy kernel against a plain fp64 reference, with a policy whose biases and log_std are all non-zero and distinct
(tests/policy_ref.py; SB3's init zeroes every bias, so a dropped or permuted bias passes a test built on it):

  (A) the sampler of every one-launch rollout form (quad, rigid, team, lane; every instantiation the C ABI dispatches to): with all weights
      zero the kernel's mean IS the head bias and its value the value bias, so the noise z = (raw - b) / exp(log_std) is recovered per entry
      and compared with Philox4x32-10 + Box-Muller in fp64 at gid = env_id_offset + i, draw = draw0 + t (wrapping past 2^32 included);
      log-probs against the fp64 formula; every output row of the caller's width written, the ragged last workgroup included;
  (B) the MLP part of every form: the kernel's mean (raw - exp(log_std) z_fp64) and value on the published observation rows against the
      fp64 model of the kernel's own rounding (bf16 operands, two-part first layer for the rigid vehicles), by quantiles per column;
  (C) the fp32-grade kernels at all five (obs, action) shapes: amenv_policy_forward / amenv_policy_forward_mfma against forward_fp64,
      amenv_ppo_mlp_step's gradient against fp64 autograd, per parameter block as well;
  (D) amenv_gaussian_act at 4..7 actions against the fp64 normals (non-zero env_id_offset, seed >= 2^32, draw near 2^32)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import ActorCritic, MinibatchStep, gaussian_act
from tests.policy_ref import (HEAD_BIAS, LOG_STD, VALUE_BIAS, forward_bf16_model, forward_fp64, gaussian_logp_fp64, nondegenerate_policy,
                              philox_normals_fp64)

pytestmark = pytest.mark.gpu

W32 = 2 ** 32

# (id, form, vehicle, task, waypoints, n, joints, axes, env_id_offset, seed, draw0, normaliser).  All batch sizes are ragged (not a
# multiple of the workgroup's envs).  Instantiations (amenv_capi_policy.hip amenv_rollout_policy / launch_lane_policy_k, amenv_rigid_policy_host.hpp launch_rigid_policy_k):
#   quad  <NROT>                    : rigid vehicle, v2, one waypoint, default workgroup size
#   rigid <NROT,KW,VAR,NORM,NE>     : NE 16 up to 6144 envs, 64 up to 24576, 128 above
#   team  <6,OCC>                   : 3-joint z,x,x arm, one waypoint, up to 6144 envs (the lane-team step family); OCC 2 above 4096
#   lane  <6,EW,KW,PNJ>             : every other arm; EW 2 above 16384 envs
CONFIGS = [
    ("quad4-v2-300", "quad", "quad", "v2", 1, 300, 0, None, 0, 77, 5, False),
    ("quad4-v2-4096-off5e9", "quad", "quad", "v2", 1, 4100, 0, None, 5_000_000_000, 78, W32 - 5, False),
    ("quad6-v2-1000", "quad", "hexa", "v2", 1, 1000, 0, None, 0, 79, 11, False),
    ("rigid4-v1s-300-ne16", "rigid", "quad", "v1_scaled", 1, 300, 0, None, 0, 80, 5, False),
    ("rigid4-v1r-12000-ne64", "rigid", "quad", "v1_raw", 1, 12001, 0, None, 0, 81, 7, False),
    ("rigid6-v1r-40000-ne128", "rigid", "hexa", "v1_raw", 1, 40003, 0, None, 3_000_000_017, W32 + 82, W32 - 5, False),
    ("rigid4-v2-3wp-3000", "rigid", "quad", "v2", 3, 3001, 0, None, 0, 83, 5, False),
    ("rigid4-v1r-4096-norm", "rigid", "quad", "v1_raw", 1, 4097, 0, None, 0, 84, 9, True),
    ("rigid6-v2-20000-norm", "rigid", "hexa", "v2", 1, 20001, 0, None, 0, 85, 9, True),
    ("team-300-occ1", "team", "hexa_arm", "v2", 1, 300, 3, None, 0, 86, 5, False),
    ("team-6000-occ2", "team", "hexa_arm", "v2", 1, 6001, 3, None, 12345, 0x1_2345_6789, W32 - 5, False),
    ("lane-nj3-20000-ew2", "lane", "hexa_arm", "v2", 1, 20001, 3, None, 0, 87, 5, False),
    ("lane-nj1-300", "lane", "hexa_arm", "v2", 1, 300, 1, None, 0, 88, 5, False),
    ("lane-nj2-20000-off", "lane", "hexa_arm", "v2", 1, 20001, 2, None, 7 * 2 ** 14, W32 + 89, W32 - 5, False),
    ("lane-nj3-4wp-3000", "lane", "hexa_arm", "v2", 4, 3001, 3, None, 0, 90, 5, False),
    ("lane-nj3-zyx-3000", "lane", "hexa_arm", "v2", 1, 3001, 3, "zyx", 0, 91, 5, False),
    ("lane-nj2-2wp-3000", "lane", "hexa_arm", "v2", 2, 3001, 2, None, 0, 92, 5, False),
]
IDS = [c[0] for c in CONFIGS]


def _env(cfg_row):
    _, form, vehicle, task, K, n, nj, axes, off, _, _, _ = cfg_row
    if nj == 0:
        env = amd.GpuWaypointEnv(n, vehicle=vehicle, task=task, num_waypoints=K, seed=4, max_episode_steps=60, env_id_offset=off)
    else:
        cfg = L.default_config("hexa_arm", n, n_joints=nj)
        cfg.seed = 4
        cfg.env_id_offset = off
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
        env = amd.GpuWaypointEnv(n, config=cfg)
    # the team form runs where the step runs the lane-team kernel for the caller's own 3-joint arm; a shorter arm there takes the lane form
    assert ("step_kernel_team" in env.kernel_name and "-joint arm" not in env.kernel_name) == (form == "team"), env.kernel_name
    assert (env.obs_dim, env.act_dim) == ((17 if task != "v2" else 20, 4) if nj == 0 else (23 + 2 * nj, 4 + nj))
    return env


def _nan_buffers(T, n, od, A, dev):
    """Every output filled with NaN (dones with 0xFF) first: a row the kernel does not write stays visible."""
    nan = float("nan")
    return dict(obs=torch.full((T + 1, n, od), nan, device=dev), actions=torch.full((T, n, A), nan, device=dev), logp=torch.full((T, n), nan, device=dev),
                values=torch.full((T, n), nan, device=dev), rewards=torch.full((T, n), nan, device=dev),
                dones=torch.full((T, n), 0xFF, dtype=torch.uint8, device=dev))


def _rollout(cfg_row, pol, T):
    """Reset the env (and warm a normaliser up to non-trivial statistics), then one rollout into NaN-filled buffers; returns the buffers."""
    env = _env(cfg_row)
    seed, draw0, norm_on = cfg_row[9], cfg_row[10], cfg_row[11]
    od, A, n, dev = env.obs_dim, env.act_dim, env.num_envs, env.device
    o0 = env.reset().clone()
    kw = {}
    if norm_on:
        norm = ObsNormalizer(od)
        norm.update(o0)
        warm = _nan_buffers(8, n, od, A, dev)
        env.rollout_policy(pol.flat_param, 8, seed + 1, 0, obs_normalizer=norm, **warm)
        kw = dict(obs_normalizer=norm)
    b = _nan_buffers(T, n, od, A, dev)
    env.rollout_policy(pol.flat_param, T, seed, draw0, **b, **kw)
    torch.cuda.synchronize()
    for k, v in b.items():
        if k == "dones":
            assert bool(((v == 0) | (v == 1)).all()), "a dones entry was not written"
        else:
            assert not bool(torch.isnan(v).any()), f"a row of {k} was not written"
    if norm_on:
        norm.close()
    env.close()
    return b


def _zero_weights(pol):
    with torch.no_grad():
        for m in pol.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.zero_()
    return pol


def _z_ref(cfg_row, T, n, A):
    off, seed, draw0 = cfg_row[8], cfg_row[9], cfg_row[10]
    return philox_normals_fp64(seed, off + np.arange(n)[None, :], (draw0 + np.arange(T))[:, None], A)


# Bounds on |z_kernel - z_fp64| beyond the fp32 rounding of raw and std (accounted for per entry by _raw_rounding).  u1, u2 are exact in fp32
# (24-bit integers x 2^-24) and rad <= sqrt(2 ln 2^24) = 5.77.  Both kernels round the angle 2 pi u2 to fp32: up to 2 x 2^-24 x 2 pi of
# argument, <= 2.2e-6 in z; rad and the final product add a few ulp of |z| (<= 1.4e-6).
# (D) amenv_gaussian_act: precise logf / sqrtf / sincosf (an ulp or two each): |dz| < 2.2e-6 + 1.4e-6 < 4e-6.
Z_PRECISE_BOUND = 4e-6
# (A) the rollout kernels: v_log_f32 / v_sin_f32 / v_cos_f32 (__logf / __sinf / __cosf) and v_sqrt_f32; the sine and cosine add up to
# 2^-20 absolute on a period (<= 5.5e-6 in z), the logarithm a few ulp (relative, so rad keeps its relative accuracy as u1 -> 1): < 1e-5.
# Measured on MI355X: max 1.8e-6 (A) and 1.2e-6 (D) -- the shared fp32 rounding of the angle dominates both.
Z_FAST_BOUND = 1e-5


def _raw_rounding(raw, std, z):
    """Per-entry bound on the recovered z's error from the fp32 rounding of raw = fma(std, z, mean) (half an ulp of raw, over std) and of
    the kernel's std = expf(log_std) (an ulp or two, relative)."""
    return 2.0 ** -24 * raw.abs() / std + 2.0 ** -22 * z.abs()


@pytest.mark.parametrize("cfg_row", CONFIGS, ids=IDS)
def test_sampler_noise_and_logp_vs_fp64(cfg_row):
    """(A): all weights zero, so mean == head bias and value == value bias exactly (an MFMA on zero operands adds exact zeros); the recovered
    z against the fp64 Philox normals at gid = env_id_offset + i and draw = draw0 + t; log-probs against the fp64 formula on that z."""
    T = 12
    n = cfg_row[5]
    od = (17 if cfg_row[3] != "v2" else 20) if cfg_row[6] == 0 else 23 + 2 * cfg_row[6]
    A = 4 + cfg_row[6]
    pol = _zero_weights(nondegenerate_policy(od, A, seed=od + A, device="cuda"))
    b = _rollout(cfg_row, pol, T)
    assert torch.equal(b["values"], torch.full_like(b["values"], VALUE_BIAS)), "value != value bias"
    raw = b["actions"].double()
    ls = pol.log_std.detach().double()
    std = torch.exp(ls)
    mean = torch.tensor(HEAD_BIAS[:A], dtype=torch.float32, device=raw.device).double()
    z = (raw - mean) / std
    zr = torch.from_numpy(_z_ref(cfg_row, T, n, A)).to(raw.device)
    slack = _raw_rounding(raw, std, z)
    dz = (z - zr).abs()
    worst = float((dz - slack).max())
    lp_ref = torch.from_numpy(gaussian_logp_fp64(z.cpu().numpy(), ls.cpu().numpy())).to(raw.device)
    dlp = (b["logp"].double() - lp_ref).abs()
    lp_tol = 2e-6 * (1.0 + lp_ref.abs()) + (z.abs() * slack).sum(-1)
    print(f"\n[A] {cfg_row[0]}: max |dz| {float(dz.max()):.2e} (beyond the raw rounding {worst:.2e}), 99.99% {float(dz.flatten().quantile(0.9999)):.2e}; "
          f"max |dlogp| {float(dlp.max()):.2e}, max |dlogp| / (1 + |logp|) {float((dlp / (1 + lp_ref.abs())).max()):.2e}")
    assert worst <= Z_FAST_BOUND, worst
    assert bool((dlp <= lp_tol).all()), float((dlp - lp_tol).max())


def _mlp_recovered(b, pol, cfg_row, T, n, A):
    ls = pol.log_std.detach().double()
    zr = torch.from_numpy(_z_ref(cfg_row, T, n, A)).to(b["actions"].device)
    return b["actions"].double() - torch.exp(ls) * zr


@pytest.mark.parametrize("cfg_row", CONFIGS, ids=IDS)
def test_rollout_mlp_vs_bf16_model(cfg_row):
    """(B): nondegenerate_policy; the kernel's mean (raw - exp(log_std) z_fp64) and value of every step against forward_bf16_model on the
    published rows (with the normaliser inside the launch: the normalised rows, the MLP's input bit for bit).  Single bf16 rounding flips of an
    activation (tanh on v_exp / v_rcp vs the exact tanh; fp32 vs fp64 sums) make single rows differ: quantiles per column."""
    T = 24
    n = cfg_row[5]
    two_part = cfg_row[1] in ("quad", "rigid")
    od = (17 if cfg_row[3] != "v2" else 20) if cfg_row[6] == 0 else 23 + 2 * cfg_row[6]
    A = 4 + cfg_row[6]
    pol = nondegenerate_policy(od, A, seed=od + A, device="cuda")
    b = _rollout(cfg_row, pol, T)
    mean_k = _mlp_recovered(b, pol, cfg_row, T, n, A).reshape(T * n, A)
    val_k = b["values"].double().reshape(-1)
    obs = b["obs"][:T].reshape(T * n, od)
    m_ref, v_ref = forward_bf16_model(pol, obs, two_part)
    m64, v64 = forward_fp64(pol, obs)
    cols = [(f"mean[{k}]", mean_k[:, k], m_ref[:, k], m64[:, k]) for k in range(A)] + [("value", val_k, v_ref, v64)]
    report = []
    fails = []
    for name, got, ref, r64 in cols:
        scale = max(1.0, float(ref.abs().max()))
        e = (got - ref).abs() / scale
        q50, q999, mx = float(e.median()), float(e.quantile(0.999)), float(e.max())
        e64 = float((got - r64).abs().max()) / scale
        report.append(f"{name} {q50:.1e}/{q999:.1e}/{mx:.1e} fp64 {e64:.1e}")
        if not (q50 <= 1e-5 and q999 <= 5e-4 and mx <= 5e-3 and e64 < 3e-2):
            fails.append((name, q50, q999, mx, e64))
    print(f"\n[B] {cfg_row[0]}: |kernel - bf16 model| / scale median / 99.9% / max: " + "; ".join(report))
    assert not fails, fails


# ---- (C) the fp32-grade kernels at all five shapes --------------------------------------------------------------------------------------
SHAPES = [(20, 4), (17, 4), (29, 7), (25, 5), (27, 6)]


@pytest.mark.parametrize("D,A", SHAPES)
@pytest.mark.parametrize("n", [1, 1000, 32768])
def test_forward_kernels_vs_fp64(D, A, n):
    """amenv_policy_forward (VALU) and amenv_policy_forward_mfma, both at every n, within 2e-5 of the scale of forward_fp64."""
    pol = nondegenerate_policy(D, A, seed=D * 10 + A, device="cuda")
    obs = torch.randn(n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(D + n)) * 1.5
    m64, v64 = forward_fp64(pol, obs)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ws = torch.empty(L.load().amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp = pol.flat_param.detach()
    for form in ("valu", "mfma"):
        m, v = torch.full((n, A), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        if form == "valu":
            rc = L.load().amenv_policy_forward(p(fp), D, A, p(obs), n, p(m), p(v), stream)
        else:
            rc = L.load().amenv_policy_forward_mfma(p(fp), D, A, p(obs), n, p(m), p(v), p(ws), stream)
        assert rc == 0, form
        torch.cuda.synchronize()
        em = float((m.double() - m64).abs().max()) / max(1.0, float(m64.abs().max()))
        ev = float((v.double() - v64).abs().max()) / max(1.0, float(v64.abs().max()))
        assert em < 2e-5 and ev < 2e-5, (form, em, ev)


@pytest.mark.parametrize("D,A", SHAPES)
def test_fused_mlp_step_vs_fp64_autograd(D, A):
    """amenv_ppo_mlp_step with non-zero biases at every shape, ragged n: against the same loss differentiated in fp64, the error is at most
    max(4 x torch fp32's, 2e-6) of the largest entry (test_fused_mlp_step_is_as_accurate_as_fp32_autograd's bar), and every parameter block
    on its own at most max(4 x torch fp32's error in that block, 1e-5 x the block's largest entry)."""
    n = 20011
    pol = nondegenerate_policy(D, A, seed=D * 10 + A + 1, device="cuda")
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-3)
    g = torch.Generator(device="cuda").manual_seed(D + A)
    obs = torch.randn(n, D, device="cuda", generator=g) * 0.7
    with torch.no_grad():
        mean = pol.action_net(pol.mlp_extractor.policy_net(obs))
    actions = mean + torch.exp(pol.log_std.detach()) * torch.randn(n, A, device="cuda", generator=g)
    with torch.no_grad():
        _, logp, _ = pol.evaluate_actions(obs, actions)
    old_logp = logp + 0.15 * torch.randn(n, device="cuda", generator=g)
    adv = torch.randn(n, device="cuda", generator=g) * 3.0 + 0.5
    ret = torch.randn(n, device="cuda", generator=g) * 2.0 + VALUE_BIAS
    grads = {}
    for fused in (False, True):
        step = MinibatchStep(pol, opt, clip_range=0.2, ent_coef=5e-4, vf_coef=0.5, use_graph=False, fused_loss=False, fused_mlp=fused)
        assert step.fused_mlp == fused
        pol.flat_grad.zero_()
        step._forward_backward(obs, actions, old_logp, adv, ret)
        torch.cuda.synchronize()
        grads[fused] = pol.flat_grad.double().clone()
        s = step.stats[:4].clone()
    pol64 = ActorCritic(D, A).cuda().double()
    pol64.load_state_dict({k: v.double() for k, v in pol.state_dict().items() if k in pol64.state_dict()})
    a64 = adv.double()
    a64 = (a64 - a64.mean()) / (a64.std() + 1e-8)
    values, logp64, ent = pol64.evaluate_actions(obs.double(), actions.double())
    ratio = torch.exp(logp64 - old_logp.double())
    loss = -torch.min(a64 * ratio, a64 * ratio.clamp(0.8, 1.2)).mean() - 5e-4 * ent.mean() + 0.5 * ((ret.double() - values) ** 2).mean()
    g64 = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(pol64.parameters()))])
    scale = float(g64.abs().max())
    e_torch, e_fused = float((grads[False] - g64).abs().max()) / scale, float((grads[True] - g64).abs().max()) / scale
    print(f"\n[C] ({D},{A}) n {n}: gradient error vs fp64 autograd / largest entry: torch fp32 {e_torch:.2e}, fused kernel {e_fused:.2e}")
    assert e_fused < max(4.0 * e_torch, 2e-6), (e_fused, e_torch)
    assert 0.02 < float(s[3]) < 0.9                                         # clip fraction: both branches of the clipped objective ran
    off, worst = 0, []
    for name, p_ in pol.named_parameters():
        k = p_.numel()
        blk = float(g64[off:off + k].abs().max())
        et = float((grads[False][off:off + k] - g64[off:off + k]).abs().max())
        ef = float((grads[True][off:off + k] - g64[off:off + k]).abs().max())
        worst.append(f"{name} {ef / blk:.1e} (torch {et / blk:.1e})")
        assert blk > 0 and ef <= max(4.0 * et, 1e-5 * blk), (name, ef, et, blk)
        off += k
    print("    per block, fused (torch) error / block's largest entry: " + "; ".join(worst))


# ---- (D) amenv_gaussian_act -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [4, 5, 6, 7])
def test_gaussian_act_vs_fp64_normals(A):
    """amenv_gaussian_act with distinct means and log_std, env_id_offset 3e9 + 7, seed >= 2^32, draw 2^32 - 2: z per entry against the fp64
    Philox normals (precise logf / sincosf: a few ulp), log-probs against the fp64 formula, the clip exact, every row written (n ragged)."""
    n, off, seed, draw = 20011, 3_000_000_007, 0x9_8765_4321, W32 - 2
    dev = "cuda"
    mean = (torch.randn(n, A, device=dev, generator=torch.Generator(device=dev).manual_seed(A)) * 0.5).contiguous()
    log_std = torch.tensor(LOG_STD[:A], device=dev)
    low, high = torch.tensor([0.0] + [-1.0] * (A - 1), device=dev), torch.tensor([2.0] + [1.0] * (A - 1), device=dev)
    raw, clipped, logp = (torch.full((n, A), float("nan"), device=dev), torch.full((n, A), float("nan"), device=dev),
                          torch.full((n,), float("nan"), device=dev))
    gaussian_act(mean, log_std, low, high, raw, clipped, logp, seed=seed, draw=draw, env_id_offset=off)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(raw).any() or torch.isnan(clipped).any() or torch.isnan(logp).any())
    assert torch.equal(clipped, torch.max(torch.min(raw, high), low))
    std = torch.exp(log_std.double())
    z = (raw.double() - mean.double()) / std
    zr = torch.from_numpy(philox_normals_fp64(seed, off + np.arange(n), draw, A)).to(dev)
    slack = _raw_rounding(raw.double(), std, z)
    dz = (z - zr).abs()
    lp_ref = torch.from_numpy(gaussian_logp_fp64(z.cpu().numpy(), LOG_STD[:A])).to(dev)
    dlp = (logp.double() - lp_ref).abs()
    print(f"\n[D] A {A}: max |dz| {float(dz.max()):.2e} (beyond the raw rounding {float((dz - slack).max()):.2e}); max |dlogp| {float(dlp.max()):.2e}")
    assert float((dz - slack).max()) <= Z_PRECISE_BOUND
    assert bool((dlp <= 2e-6 * (1.0 + lp_ref.abs()) + (z.abs() * slack).sum(-1)).all())
