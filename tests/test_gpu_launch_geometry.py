"""Every launch-geometry threshold of the training-side kernels (everything behind the C ABI that is not an env step) against fp64.

Each launcher in csrc/amenv_capi*.hip caps its grid and loops inside the kernel beyond the cap, or switches its block size at a batch size.
GEOMETRY below is the one table of those thresholds with the n values that straddle them; tests/test_launch_geometry_cpu.py recomputes every
threshold from the sources, so a changed cap fails there instead of silently un-testing a loop.  Every case here fills its outputs with NaN,
keeps 64 NaN guard rows behind each output, asserts that the guards are untouched and every row below n written, and compares with an fp64
reference of the same operation (tests/policy_ref.py, oracle.gae_reference, the RunningMeanStd restatement of tests/test_gpu_obsnorm.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import ActorCritic, MinibatchStep
from tests.policy_ref import LOG_STD, VALUE_BIAS, forward_fp64, gaussian_logp_fp64, nondegenerate_policy, philox_normals_fp64

pytestmark = pytest.mark.gpu

GUARD = 64          # NaN rows behind every output
CLIP, ENT_COEF, VF_COEF = 0.2, 5e-4, 0.5
W32 = 2 ** 32

# ---- the tested sizes ---------------------------------------------------------------------------------------------------------------------
FWD_BOTH_N = (32769, 32901, 65541)                      # amenv_policy_forward_mfma, mean and value
FWD_ONE_N = (1000, 65536, 65537, 65669)                 # one output (and the two-output call it must equal bit for bit)
FWD_VALU_N = (1, 65)                                    # amenv_policy_forward
LOSS_N = (1, 2, 255, 256, 257, 262144, 262145, 600001)  # amenv_ppo_loss_grad
STEP_N = (1, 33, 129, 896, 1025, 16384, 16385, 262221)  # amenv_ppo_mlp_step
STEP_GATHER_N = (16385, 262221)                         # ... with an index gather out of STEP_GATHER_ROWS rows
STEP_GATHER_ROWS = 300000
ADAM_N = (1, 3, 4, 5, 1023, 1024, 1025, 65535, 65536, 65537)
GAE_TN = ((1, 65536), (3, 65537), (2, 1))
ACT_N = (1, 65536, 65537)
# (dim, n) of amenv_obsnorm_update / amenv_obsnorm_apply
OBSNORM_DIM_N = ((1, 1), (1, 1000), (25, 300), (27, 300), (29, 1), (29, 9039), (29, 9040), (29, 18078), (29, 18079), (64, 100), (257, 50),
                 (1024, 3), (1024, 300))

# (row, kernel, what is capped, threshold = the largest size the first round / the smaller configuration serves, the tested sizes).
# tests/test_launch_geometry_cpu.py recomputes every threshold from csrc/ and asserts sizes on both sides of each.
GEOMETRY = [
    ("fwd_mfma_both", "amenv_policy_forward_mfma", "mean + value: 512 / 2 workgroups x 4 tiles x 32 rows per round", 32768, FWD_ONE_N + FWD_BOTH_N),
    ("fwd_mfma_both_round2", "amenv_policy_forward_mfma", "mean + value: end of the second round", 65536, FWD_ONE_N + FWD_BOTH_N),
    ("fwd_mfma_one", "amenv_policy_forward_mfma", "one output: 512 workgroups x 4 tiles x 32 rows per round", 65536, FWD_ONE_N),
    ("fwd_valu_block", "amenv_policy_forward", "64 rows per workgroup", 64, FWD_VALU_N),
    ("loss_round", "amenv_ppo_loss_grad", "kPpoMaxBlocks x kPpoBlock samples per grid-stride round", 262144, LOSS_N),
    ("loss_round2", "amenv_ppo_loss_grad", "end of the second round", 524288, LOSS_N),
    ("loss_block", "amenv_ppo_loss_grad", "one workgroup (kPpoBlock lanes)", 256, LOSS_N),
    ("step_slab", "amenv_ppo_mlp_step", "one workgroup = one slab: 4 tiles x 32 samples", 128, STEP_N),
    ("step_reduce_groups", "amenv_ppo_mlp_step", "mlp_grad_reduce_kernel: at most one slab per group (kRedGroups slabs)", 1024, STEP_N),
    ("step_round", "amenv_ppo_mlp_step", "128 workgroups x 4 tiles x 32 samples per round", 16384, STEP_N),
    ("step_adv_round", "amenv_ppo_mlp_step", "advantage partials: kPpoMaxBlocks x kPpoBlock samples per round", 262144, STEP_N),
    ("step_adv_round_gather", "amenv_ppo_mlp_step", "the same with the index gather", 262144, STEP_GATHER_N),
    ("adam_float4", "amenv_ppo_adam_step", "no float4 part of the norm pass below 4 entries", 3, ADAM_N),
    ("adam_block", "amenv_ppo_adam_step", "one workgroup (kAdamBlock entries)", 1024, ADAM_N),
    ("adam_grid", "amenv_ppo_adam_step", "kAdamMaxBlocks x kAdamBlock entries: longer slices per workgroup beyond", 65536, ADAM_N),
    ("gae_block", "amenv_gae", "64-lane workgroups up to here, 256 beyond", 65536, tuple(n for _, n in GAE_TN)),
    ("act_block", "amenv_gaussian_act", "64-lane workgroups up to here, 256 beyond", 65536, ACT_N),
    ("obsnorm_update_grid", "amenv_obsnorm_update", "1024 workgroups x 256 elements at dim 29 (rows)", 9039, tuple(n for d, n in OBSNORM_DIM_N if d == 29)),
    ("obsnorm_apply_grid", "amenv_obsnorm_apply", "2048 workgroups x 256 elements at dim 29 (rows)", 18078, tuple(n for d, n in OBSNORM_DIM_N if d == 29)),
    ("obsnorm_block_dim", "amenv_obsnorm_update", "dims up to the 256-thread workgroup: one trip of the LDS loops", 256, tuple(d for d, _ in OBSNORM_DIM_N)),
    ("obsnorm_max_dim", "amenv_obsnorm_create", "largest accepted dim (the next one is refused)", 1024, tuple(d for d, _ in OBSNORM_DIM_N) + (1025,)),
]


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(rows, *tail, dtype=torch.float32):
    """An output of `rows` rows with GUARD rows behind it, all NaN."""
    return torch.full((rows + GUARD,) + tail, float("nan"), dtype=dtype, device="cuda")


def _written(buf, rows, name):
    """Every row below `rows` written, the guard rows behind untouched; returns the written part."""
    assert not bool(torch.isnan(buf[:rows]).any()), f"{name}: a row below n was not written"
    assert bool(torch.isnan(buf[rows:]).all()), f"{name}: a guard row was written"
    return buf[:rows]


def _cpu_gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * 1000003 ** i for i, k in enumerate(key)) % (2 ** 63))


def _randn(g, *shape):
    """Inputs are drawn on the host (the same on every machine) and copied over."""
    return torch.randn(*shape, generator=g)


def _off_the_clip_edges(noise):
    """old_logp = logp + noise makes the ratio exp(-noise).  The clipped objective's gradient jumps where the ratio crosses 1 +- CLIP, so a
    sample within fp32 rounding of an edge (about one in 600,000 samples is) would compare the side the kernel's rounding picked, not its
    arithmetic: samples within 1e-4 of an edge are moved 1 % away from it."""
    r = torch.exp(-noise.double())
    near = ((r - (1.0 - CLIP)).abs() < 1e-4) | ((r - (1.0 + CLIP)).abs() < 1e-4)
    return torch.where(near, noise + 0.01, noise)


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
FWD_MAIN_SHAPES = [(17, 4), (29, 7)]
FWD_OTHER_SHAPES = [(20, 4), (25, 5), (27, 6)]
FWD_CASES = ([(D, A, n, False) for D, A in FWD_MAIN_SHAPES for n in FWD_BOTH_N] + [(D, A, 32901, False) for D, A in FWD_OTHER_SHAPES] +
             [(D, A, n, True) for D, A in FWD_MAIN_SHAPES for n in FWD_ONE_N] + [(D, A, 65537, True) for D, A in FWD_OTHER_SHAPES])


def _forward(form, pol, obs, n, want_mean, want_value, ws):
    D, A = pol.obs_dim, pol.act_dim
    m = _nan(n, A) if want_mean else None
    v = _nan(n) if want_value else None
    fp = pol.flat_param.detach()
    if form == "mfma":
        rc = L.load().amenv_policy_forward_mfma(_p(fp), D, A, _p(obs), n, _p(m), _p(v), _p(ws), _stream())
    else:
        rc = L.load().amenv_policy_forward(_p(fp), D, A, _p(obs), n, _p(m), _p(v), _stream())
    assert rc == 0, (form, want_mean, want_value)
    torch.cuda.synchronize()
    return (_written(m, n, "mean") if want_mean else None), (_written(v, n, "value") if want_value else None)


def _forward_case(form, D, A, n, single):
    pol = nondegenerate_policy(D, A, seed=D * 10 + A, device="cuda")
    obs = (_randn(_cpu_gen(D, n), n, D) * 1.5).cuda()
    m64, v64 = forward_fp64(pol, obs)
    ws = torch.empty(L.load().amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device="cuda")
    m, v = _forward(form, pol, obs, n, True, True, ws)
    em = float((m.double() - m64).abs().max()) / max(1.0, float(m64.abs().max()))
    ev = float((v.double() - v64).abs().max()) / max(1.0, float(v64.abs().max()))
    print(f"\n[forward {form}] ({D},{A}) n {n}: |mean - fp64| / scale {em:.2e}, |value - fp64| / scale {ev:.2e}")
    assert em < 2e-5 and ev < 2e-5, (form, em, ev)
    if single:   # the production form of ActorCritic.actor() / critic(): the other net's workgroups return at once
        m1, none = _forward(form, pol, obs, n, True, False, ws)
        assert none is None and torch.equal(m1, m), "mean-only differs from the two-output call"
        none, v1 = _forward(form, pol, obs, n, False, True, ws)
        assert none is None and torch.equal(v1, v), "value-only differs from the two-output call"


@pytest.mark.parametrize("D,A,n,single", FWD_CASES)
def test_forward_mfma_beyond_one_round(D, A, n, single):
    """amenv_policy_forward_mfma past the first trip of its tile loop (two outputs: n > 32,768; one output: n > 65,536), ragged last tiles,
    within 2e-5 of the scale of forward_fp64; the one-output calls bit-identical to the same rows of the two-output call."""
    _forward_case("mfma", D, A, n, single)


@pytest.mark.parametrize("D,A", FWD_MAIN_SHAPES)
@pytest.mark.parametrize("n", FWD_VALU_N)
def test_forward_valu_single_output(D, A, n):
    """amenv_policy_forward with one output (NULL for the other) equals its two-output call bit for bit, at one row and one row past a workgroup."""
    _forward_case("valu", D, A, n, True)


# ---- loss ---------------------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(A, n) for A in (4, 7) for n in LOSS_N] + [(5, 262145), (6, 262145)]


def _loss_inputs(A, n, const_adv=None):
    """Synthetic network outputs and rollout data; old_logp = logp + N(0, 0.3^2), so about half of the ratios leave the clip range."""
    g = _cpu_gen(A, n, 7)
    mean = _randn(g, n, A) * 0.5
    log_std = torch.tensor(LOG_STD[:A])
    actions = mean + torch.exp(log_std) * 1.5 * _randn(g, n, A)
    value = _randn(g, n) * 2.0
    ret = _randn(g, n) * 10.0
    adv = _randn(g, n) * 3.0 + 0.5 if const_adv is None else torch.full((n,), const_adv)
    noise = _off_the_clip_edges(0.3 * _randn(g, n))
    mean, log_std, actions, value, ret, adv, noise = (t.cuda().contiguous() for t in (mean, log_std, actions, value, ret, adv, noise))
    z = (actions.double() - mean.double()) * torch.exp(-log_std.double())
    logp = torch.from_numpy(gaussian_logp_fp64(z.cpu().numpy(), log_std.double().cpu().numpy())).cuda()
    return mean, value, log_std, actions, (logp + noise.double()).float().contiguous(), adv, ret


def _loss_kernel(inp, n, A, normalize):
    mean, value, log_std, actions, old_logp, adv, ret = inp
    d_mean, d_value, d_ls, stats = _nan(n, A), _nan(n), _nan(A), _nan(4)
    ws = torch.empty(L.load().amenv_ppo_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    rc = L.load().amenv_ppo_loss_grad(_p(mean), _p(value), _p(log_std), _p(actions), _p(old_logp), _p(adv), _p(ret), n, A, CLIP, ENT_COEF, VF_COEF,
                                      1 if normalize else 0, _p(d_mean), _p(d_value), _p(d_ls), _p(stats), _p(ws), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _written(d_mean, n, "d_mean"), _written(d_value, n, "d_value"), _written(d_ls, A, "d_log_std"), _written(stats, 4, "stats")


def _loss_fp64(inp, n, normalize):
    """SB3's loss in fp64, differentiated by autograd with respect to mean, value and log_std; the four reported scalars."""
    mean, value, log_std, actions, old_logp, adv, ret = inp
    m, v, ls = (t.double().clone().requires_grad_(True) for t in (mean, value, log_std))
    a = adv.double()
    if normalize and n > 1:                                                        # SB3: only where the minibatch has more than one sample
        a = (a - a.mean()) / (a.std() + 1e-8)
    z = (actions.double() - m) * torch.exp(-ls)
    logp = (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    ratio = torch.exp(logp - old_logp.double())
    pl = -torch.min(a * ratio, a * ratio.clamp(1.0 - CLIP, 1.0 + CLIP)).mean()
    vl = ((ret.double() - v) ** 2).mean()
    el = -(0.5 + 0.5 * math.log(2.0 * math.pi) + ls).sum()
    gm, gv, gl = torch.autograd.grad(pl + ENT_COEF * el + VF_COEF * vl, [m, v, ls])
    stats = torch.stack([pl.detach(), vl.detach(), el.detach(), ((ratio.detach() - 1.0).abs() > CLIP).double().mean()])
    return gm, gv, gl, stats


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("A,n", LOSS_CASES)
def test_loss_grad_kernel_vs_fp64_autograd(A, n, normalize):
    """amenv_ppo_loss_grad on its own (no MLP): d_mean, d_value, d_log_std within 2e-5 of the largest reference entry of each output, the
    four scalars within 1e-4, from one sample to past two grid-stride rounds of 1,024 x 256 samples."""
    inp = _loss_inputs(A, n)
    outs = _loss_kernel(inp, n, A, normalize)
    refs = _loss_fp64(inp, n, normalize)
    errs = []
    for name, got, ref in zip(("d_mean", "d_value", "d_log_std"), outs[:3], refs[:3]):
        errs.append((name, float((got.double() - ref).abs().max()), float(ref.abs().max())))
    es = float(((outs[3].double() - refs[3]).abs() / refs[3].abs().clamp(min=1e-3)).max())
    print(f"\n[loss] A {A} n {n} normalize {normalize}: " + ", ".join(f"{k} {e:.2e} of {sc:.2e}" for k, e, sc in errs) + f", stats {es:.2e}, clip fraction {float(refs[3][3]):.3f}")
    for name, e, sc in errs:                                                        # (a lone clipped sample has d_mean = 0: then exactly)
        assert e <= 2e-5 * sc, (name, e, sc)
    assert es < 1e-4, (outs[3], refs[3])
    if n >= 255:
        assert 0.05 < float(refs[3][3]) < 0.95                                     # both clipped and unclipped samples present
    if n == 1 and normalize:                                                       # SB3's n > 1 rule: the advantage is used as it is
        raw = _loss_kernel(inp, n, A, False)
        assert all(torch.equal(x, y) for x, y in zip(outs, raw))


@pytest.mark.parametrize("A", [4, 7])
def test_loss_grad_kernel_constant_advantage(A):
    """All advantages equal (variance 0, the fmax(var, 0) path) with normalisation on: the normalised advantage is exactly 0, so d_mean and
    d_log_std + ent_coef are exactly zero and nothing is NaN or Inf; the value part is unaffected."""
    n = 10007
    inp = _loss_inputs(A, n, const_adv=1.7)
    d_mean, d_value, d_ls, stats = _loss_kernel(inp, n, A, True)
    for t in (d_mean, d_value, d_ls, stats):
        assert bool(torch.isfinite(t).all())
    assert not bool(d_mean.any()), float(d_mean.abs().max())
    assert not bool((d_ls + ENT_COEF).any()), d_ls
    gm, gv, gl, ref_stats = _loss_fp64(inp, n, True)
    assert float((d_value.double() - gv).abs().max()) < 2e-5 * float(gv.abs().max())
    assert float(stats[0]) == 0.0 and abs(float(ref_stats[0])) < 1e-6
    assert float(((stats[1:].double() - ref_stats[1:]).abs() / ref_stats[1:].abs().clamp(min=1e-3)).max()) < 1e-4


# ---- fused minibatch step -------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = [(17, 4), (29, 7)]


def _step_problem(D, A, rows, key):
    """Policy and `rows` rows of rollout data (host-drawn): ratios spread around 1, so both sides of the clip fire."""
    pol = nondegenerate_policy(D, A, seed=D * 10 + A + 1, device="cuda")
    g = _cpu_gen(D, A, rows, key)
    obs = (_randn(g, rows, D) * 0.7).cuda()
    e1, e2 = _randn(g, rows, A).cuda(), _off_the_clip_edges(0.15 * _randn(g, rows)).cuda()
    adv = (_randn(g, rows) * 3.0 + 0.5).cuda()
    ret = (_randn(g, rows) * 2.0 + VALUE_BIAS).cuda()
    with torch.no_grad():
        mean = pol.action_net(pol.mlp_extractor.policy_net(obs))
        actions = (mean + torch.exp(pol.log_std.detach()) * e1).contiguous()
        _, logp, _ = pol.evaluate_actions(obs, actions)
    return pol, (obs, actions, (logp + e2).contiguous(), adv, ret)


def _guarded_fused(step, pol, call):
    """Run `call` with the gradient and the stats landing in NaN-filled buffers with guard entries behind; returns (grad, stats[:4])."""
    total = pol.flat_grad.numel()
    gbuf, sbuf = _nan(total), _nan(5)
    keep = pol.flat_grad, step.stats
    pol.flat_grad, step.stats = gbuf[:total], sbuf[:5]
    try:
        call()
        torch.cuda.synchronize()
    finally:
        pol.flat_grad, step.stats = keep
    return _written(gbuf, total, "flat_grad").clone(), _written(sbuf, 4, "stats").clone()   # (stats[4], the gradient norm, is Adam's)


@pytest.mark.parametrize("D,A", STEP_SHAPES)
@pytest.mark.parametrize("n", STEP_N)
def test_fused_mlp_step_slab_counts_vs_fp64_autograd(D, A, n):
    """amenv_ppo_mlp_step at 1, 2, 7, 9 and 128 slabs, at the first n past one round (workgroups 65.. see no valid sample) and past the
    advantage-partials cap: against the same loss differentiated in fp64 the error is at most max(4 x torch fp32's, 2e-6) of the largest
    entry, and every parameter block at most max(4 x torch fp32's error in that block, 1e-5 x the block's largest entry)."""
    pol, data = _step_problem(D, A, n, 1)
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-3)
    plain = MinibatchStep(pol, opt, clip_range=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF, use_graph=False, fused_loss=False, fused_mlp=False)
    assert not plain.fused_mlp
    pol.flat_grad.zero_()
    plain._forward_backward(*data)
    torch.cuda.synchronize()
    g_torch = pol.flat_grad.double().clone()
    fused = MinibatchStep(pol, opt, clip_range=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF, use_graph=False, fused_loss=False, fused_mlp=True)
    assert fused.fused_mlp
    g_fused, s = _guarded_fused(fused, pol, lambda: fused._forward_backward(*data))
    g_fused = g_fused.double()
    obs, actions, old_logp, adv, ret = data
    pol64 = ActorCritic(D, A).cuda().double()
    pol64.load_state_dict({k: v.double() for k, v in pol.state_dict().items() if k in pol64.state_dict()})
    a64 = adv.double()
    if n > 1:
        a64 = (a64 - a64.mean()) / (a64.std() + 1e-8)
    values, logp64, ent = pol64.evaluate_actions(obs.double(), actions.double())
    ratio = torch.exp(logp64 - old_logp.double())
    pl, vl, el = -torch.min(a64 * ratio, a64 * ratio.clamp(1.0 - CLIP, 1.0 + CLIP)).mean(), ((ret.double() - values) ** 2).mean(), -ent.mean()
    g64 = torch.cat([x.reshape(-1) for x in torch.autograd.grad(pl + ENT_COEF * el + VF_COEF * vl, list(pol64.parameters()))])
    scale = float(g64.abs().max())
    e_torch, e_fused = float((g_torch - g64).abs().max()) / scale, float((g_fused - g64).abs().max()) / scale
    print(f"\n[step] ({D},{A}) n {n}: gradient error vs fp64 autograd / largest entry: torch fp32 {e_torch:.2e}, fused kernel {e_fused:.2e}")
    ref_stats = torch.stack([pl, vl, el, ((ratio - 1.0).abs() > CLIP).double().mean()]).detach()
    es = float(((s.double() - ref_stats).abs() / ref_stats.abs().clamp(min=1e-3)).max())
    off, worst, bad = 0, [], []
    for name, p_ in pol.named_parameters():
        k = p_.numel()
        blk = float(g64[off:off + k].abs().max())
        et = float((g_torch[off:off + k] - g64[off:off + k]).abs().max())
        ef = float((g_fused[off:off + k] - g64[off:off + k]).abs().max())
        worst.append(f"{name} {ef / max(blk, 1e-300):.1e} (torch {et / max(blk, 1e-300):.1e})")
        if not (blk > 0 and ef <= max(4.0 * et, 1e-5 * blk)):
            bad.append((name, ef, et, blk))
        off += k
    print("    per block, fused (torch) error / block's largest entry: " + "; ".join(worst) + f"; stats {es:.1e}")
    assert e_fused < max(4.0 * e_torch, 2e-6), (e_fused, e_torch)
    assert not bad, bad
    assert es < 1e-4, (s, ref_stats)                                               # the loss kernel's bar for the four scalars
    if n >= 896:
        assert 0.02 < float(s[3]) < 0.9                                            # clip fraction: both branches of the clipped objective ran


@pytest.mark.parametrize("D,A", STEP_SHAPES)
@pytest.mark.parametrize("n", STEP_GATHER_N)
def test_fused_mlp_step_index_gather_beyond_one_round(D, A, n):
    """`index` draws n rows out of a 300,000-row buffer, past one round of tiles and past the advantage-partials cap: the gradient and
    the scalars equal, bit for bit, those of the contiguous call on the gathered copies."""
    pol, full = _step_problem(D, A, STEP_GATHER_ROWS, 2)
    opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-3, capturable=True)
    step = MinibatchStep(pol, opt, clip_range=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF, use_graph=False)
    assert step.fused_mlp
    idx = torch.randperm(STEP_GATHER_ROWS, generator=_cpu_gen(n, 5))[:n].cuda()
    g_idx, s_idx = _guarded_fused(step, pol, lambda: step._forward_backward_mlp(*full, idx))
    copies = [t[idx].contiguous() for t in full]
    g_cpy, s_cpy = _guarded_fused(step, pol, lambda: step._forward_backward_mlp(*copies))
    assert torch.equal(g_idx, g_cpy) and torch.equal(s_idx, s_cpy)
    assert float(g_idx.abs().max()) > 0


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.5, None])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step_sizes_around_block_and_grid(n, max_norm):
    """amenv_ppo_adam_step from one entry (no float4 part in the norm pass) over one workgroup to past the 64-workgroup cap, two calls:
    parameters and both moments against clip_grad_norm_-style scaling + torch.optim.Adam in fp64 (test_fused_adam_step_matches_torch_adam's
    tolerances), the norm against the fp64 norm, `step` + 1 per call, the ticket word back at 0, the gradient read-only."""
    g_ = _cpu_gen(n, 11)
    p_ref = (_randn(g_, n).double() * 0.3).cuda()
    leaf = p_ref.clone().requires_grad_(True)
    opt = torch.optim.Adam([leaf], lr=2e-4, eps=1e-5)
    p_hip, m, v = _nan(n), _nan(n), _nan(n)
    p_hip[:n], m[:n], v[:n] = p_ref.float(), 0.0, 0.0
    stp, gn = torch.zeros((), device="cuda"), _nan(1)
    hyper = torch.tensor([2e-4, 0.9, 0.999, 1e-5, max_norm or 0.0, 1.0], device="cuda")
    ticket = torch.zeros(1 + GUARD, dtype=torch.int32, device="cuda")
    for it in range(2):
        g = (_randn(g_, n) * (0.05 if it else 0.3)).cuda()                          # first call: norm above max_norm from ~3 entries on
        gd = g.double()
        norm = gd.norm(2)
        if max_norm is not None:
            gd = gd * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        leaf.grad = gd.clone()
        opt.step()
        gh = g.clone()
        assert gh.data_ptr() % 16 == 0
        rc = L.load().amenv_ppo_adam_step(_p(p_hip), _p(gh), _p(m), _p(v), _p(stp), n, _p(hyper), _p(gn), _p(ticket), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert abs(float(_written(gn, 1, "grad_norm")) - float(norm)) < 1e-5 * float(norm)
        assert torch.equal(gh, g)
        assert float(stp) == it + 1.0 and not bool(ticket.any())
        st = opt.state[leaf]
        assert torch.allclose(_written(m, n, "exp_avg").double(), st["exp_avg"], rtol=1e-4, atol=1e-7)
        assert torch.allclose(_written(v, n, "exp_avg_sq").double(), st["exp_avg_sq"], rtol=1e-4, atol=1e-12)
        assert float((_written(p_hip, n, "param").double() - leaf.detach()).abs().max()) < 2e-4 * 0.02
    assert float((p_hip[:n].double() - p_ref).abs().max()) > 1e-4                   # (two steps of about lr each)


# ---- GAE ------------------------------------------------------------------------------------------------------------------------------------
GAE_CASES = [(T, N, 0.995, 0.9) for T, N in GAE_TN] + [(5, 1000, 0.0, 0.9), (5, 1000, 1.0, 1.0), (5, 1000, 0.995, 0.0)]


@pytest.mark.parametrize("T,N,gamma,lam", GAE_CASES)
def test_gae_kernel_block_switch_and_extreme_discounts(T, N, gamma, lam):
    """amenv_gae on both sides of its 64 -> 256 lane switch (n_envs 65,536 | 65,537), at one env, and at gamma / lambda of 0 and 1:
    within 1e-6 of 1 + the accumulated magnitude of the recursion's terms against oracle.gae_reference."""
    from oracle import oracle as O
    from tests.test_gpu_ppo import gae_magnitude
    rng = np.random.RandomState(T * 131 + N)
    r = rng.randn(T, N).astype(np.float32) * 5
    v = rng.randn(T, N).astype(np.float32) * 50
    d = (rng.rand(T, N) < 0.05).astype(np.uint8)
    lv = rng.randn(N).astype(np.float32) * 50
    rd, vd, dd, lvd = (torch.from_numpy(x).cuda() for x in (r, v, d, lv))
    adv, ret = _nan(T * N), _nan(T * N)
    rc = L.load().amenv_gae(_p(rd), _p(vd), _p(dd), _p(lvd), _p(adv), _p(ret), T, N, gamma, lam, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    adv, ret = _written(adv, T * N, "advantages").view(T, N), _written(ret, T * N, "returns").view(T, N)
    adv_ref, ret_ref = O.gae_reference(r, v, d, lv, gamma, lam)
    mag = gae_magnitude(r, v, d, lv, gamma, lam)
    assert (np.abs(adv.cpu().numpy() - adv_ref) / (1.0 + mag)).max() < 1e-6
    assert (np.abs(ret.cpu().numpy() - ret_ref) / (1.0 + mag)).max() < 1e-6
    msk = dd != 0
    assert torch.equal(adv[msk], (rd - vd)[msk])                                   # nothing from later steps leaks past an episode end


# ---- sampler --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [4, 7])
@pytest.mark.parametrize("n", ACT_N)
def test_gaussian_act_block_switch_vs_fp64_normals(n, A):
    """amenv_gaussian_act at one env and on both sides of its 64 -> 256 lane switch, with test_gaussian_act_vs_fp64_normals's asserts."""
    from tests.test_gpu_policy_kernels_vs_fp64 import Z_PRECISE_BOUND, _raw_rounding
    off, seed, draw = 3_000_000_007, 0x9_8765_4321, W32 - 2
    mean = (_randn(_cpu_gen(n, A), n, A) * 0.5).cuda().contiguous()
    log_std = torch.tensor(LOG_STD[:A], device="cuda")
    low, high = torch.tensor([0.0] + [-1.0] * (A - 1), device="cuda"), torch.tensor([2.0] + [1.0] * (A - 1), device="cuda")
    raw, clipped, logp = _nan(n, A), _nan(n, A), _nan(n)
    rc = L.load().amenv_gaussian_act(_p(mean), _p(log_std), _p(low), _p(high), _p(raw), _p(clipped), _p(logp), n, A, seed, draw, off, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    raw, clipped, logp = _written(raw, n, "raw"), _written(clipped, n, "clipped"), _written(logp, n, "logp")
    assert torch.equal(clipped, torch.max(torch.min(raw, high), low))
    std = torch.exp(log_std.double())
    z = (raw.double() - mean.double()) / std
    zr = torch.from_numpy(philox_normals_fp64(seed, off + np.arange(n), draw, A)).cuda()
    slack = _raw_rounding(raw.double(), std, z)
    dz = (z - zr).abs()
    lp_ref = torch.from_numpy(gaussian_logp_fp64(z.cpu().numpy(), LOG_STD[:A])).cuda()
    dlp = (logp.double() - lp_ref).abs()
    assert float((dz - slack).max()) <= Z_PRECISE_BOUND
    assert bool((dlp <= 2e-6 * (1.0 + lp_ref.abs()) + (z.abs() * slack).sum(-1)).all())


# ---- observation normaliser -------------------------------------------------------------------------------------------------------------------
def _apply(nz, src, dst, n):
    rc = nz.lib.amenv_obsnorm_apply(nz._h, _p(src), _p(dst), n, nz.clip_obs, nz.epsilon, _stream())
    assert rc == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dim,n", OBSNORM_DIM_N)
def test_obsnorm_dims_and_grid_caps(dim, n):
    """amenv_obsnorm_update / _apply at dim 1, the arm widths, dims above the 256-thread workgroup up to the largest accepted one, n = 1, and
    row counts around both grid caps: three updates against the RunningMeanStd restatement (its tolerances); apply against the fp64 formula on
    the kernel's own statistics (2e-6), out of place and in place (bit-identical)."""
    from tests.test_gpu_obsnorm import RunningMeanStd
    rng = np.random.RandomState(dim + n)
    rms = RunningMeanStd(dim)
    nz = ObsNormalizer(dim)
    for it in range(3):
        x = (rng.normal(size=(n, dim)) * rng.uniform(0.1, 5, dim) + rng.uniform(-3, 3, dim) + it).astype(np.float32)
        rms.update(x.astype(np.float64))
        xd = torch.from_numpy(x).cuda()
        nz.update(xd)
        mean, var, count = nz.get()
        np.testing.assert_allclose(mean, rms.mean, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(var, rms.var, rtol=1e-8, atol=1e-10)
        assert abs(count - rms.count) < 1e-9
        out = _nan(n, dim)
        _apply(nz, xd, out, n)
        y = _written(out, n, "apply")
        want = np.clip((x.astype(np.float64) - mean) / np.sqrt(var + 1e-8), -10, 10)
        np.testing.assert_allclose(y.cpu().numpy(), want, rtol=2e-6, atol=2e-6)
        inplace = _nan(n, dim)
        inplace[:n] = xd
        _apply(nz, inplace, inplace, n)
        assert torch.equal(_written(inplace, n, "apply in place"), y)
    nz.close()


def test_obsnorm_refuses_dims_above_1024():
    with pytest.raises(L.AmenvError):
        ObsNormalizer(1025)


def test_obsnorm_nearly_constant_column():
    """A column of 1 - |eps|, eps ~ N(0, 3e-4^2) (a quaternion's w near 1; variance ~3e-8 at mean ~1): the single-pass E[x^2] - mean^2 of
    the merge kernel at its weakest.  Variance reference: two-pass numpy in longdouble.  The attainable accuracy is that of the single-pass
    formula in fp64, measured here by a sequential fp64 restatement of what the kernels do (per-column sum and sum of squares, then the merge
    formula); the kernel's error on that column may be 8 x that (its summation order differs: rounding noise of the same size).
    Measured (MI355X): restatement 1.72e-6, kernels 8.5e-9."""
    from tests.test_gpu_obsnorm import RunningMeanStd
    dim, n, col = 20, 70000, 3
    rng = np.random.RandomState(dim + n + 1)
    rms = RunningMeanStd(dim)
    nz = ObsNormalizer(dim)
    LD = np.longdouble

    def merge(state, bm, bv, bc):   # RunningMeanStd.update_from_moments on one column, in the precision of its arguments
        mean, var, count = state
        delta, tot = bm - mean, count + bc
        return mean + delta * bc / tot, (var * count + bv * bc + delta * delta * count * bc / tot) / tot, tot

    ref, seq = (LD(0), LD(1), LD(1e-4)), (0.0, 1.0, 1e-4)
    e_seq = e_ker = 0.0
    for it in range(6):
        x = (rng.normal(size=(n, dim)) * rng.uniform(0.1, 5, dim) + rng.uniform(-3, 3, dim) + it).astype(np.float32)
        x[:, col] = (1.0 - np.abs(rng.normal(size=n) * 3e-4)).astype(np.float32)
        rms.update(x.astype(np.float64))
        c = x[:, col].astype(LD)
        bm = c.mean()
        ref = merge(ref, bm, ((c - bm) ** 2).mean(), LD(n))
        c64 = x[:, col].astype(np.float64)
        s, q = float(np.cumsum(c64)[-1]), float(np.cumsum(c64 * c64)[-1])          # cumsum: strictly sequential fp64 sums
        seq = merge(seq, s / n, max(q / n - (s / n) * (s / n), 0.0), float(n))
        nz.update(torch.from_numpy(x).cuda())
        mean, var, count = nz.get()
        others = np.arange(dim) != col
        np.testing.assert_allclose(mean, rms.mean, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(var[others], rms.var[others], rtol=1e-8, atol=1e-10)
        assert abs(count - rms.count) < 1e-9
        assert abs(mean[col] - float(ref[0])) < 1e-9
        e_seq = max(e_seq, abs(float((LD(seq[1]) - ref[1]) / ref[1])))
        e_ker = max(e_ker, abs(float((LD(var[col]) - ref[1]) / ref[1])))
    nz.close()
    print(f"\n[obsnorm] nearly constant column, variance {float(ref[1]):.3e}: relative error of the sequential fp64 restatement {e_seq:.2e}, of the kernels {e_ker:.2e}")
    assert 2e-8 < float(ref[1]) < 5e-8 and e_seq > 0
    assert e_ker <= 8.0 * e_seq, (e_ker, e_seq)
