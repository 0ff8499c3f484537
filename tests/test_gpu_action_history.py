"""Action history in the rigid vehicles' observation rows (amenv_set_action_history) on the GPU.  The env part is
compared bit for bit: a handle with the history against a twin without it (columns :base, everything else it publishes) and against a
history the test keeps itself with tests/delay_ref.py and tests/history_ref.py (columns base:); rollouts and closed loops replay through
amenv_step; toggling, refusals, sharding, restore; the MLP kernels at the four new shapes under the project's own gates; one fp32 case
against the fp64 oracle."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import PPO, ActorCritic, MinibatchStep
from tests import history_ref
from tests import switch_harness as SH     # (H is the number of history rows in this file)
from tests.policy_ref import VALUE_BIAS, forward_bf16_model, forward_fp64, nondegenerate_policy, philox_normals_fp64

pytestmark = pytest.mark.gpu
SW = SH.ACTION_HISTORY

N, GID0 = 200, 1000                      # three full tiles + 8 ragged lanes; a non-zero env_id_offset
FULL = amd.ActionDelay(0, 8)
DR = amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1))
LAG = amd.RotorLag(0.015, 0.04)
NOISE = amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01)
ALL = dict(randomization=DR, rotor_lag=LAG, sensor_noise=NOISE)
H1, H2 = amd.ActionHistory(1), amd.ActionHistory(2)
HOVER = np.array([1.0, 0.0, 0.0, 0.0], np.float32)


def _env(vehicle="quad", task="v2", nwp=1, n=N, seed=4, **kw):
    kw.setdefault("env_id_offset", GID0)
    return SH.make_env(vehicle, task, nwp, n, seed, **kw)


_actions = functools.partial(SH.actions, wide=True)      # near +-1 (and 0 / 2 on the collective), so consecutive rows differ strongly
_nan_buffers = functools.partial(SH.buffers, fill=float("nan"))
_step_all, _same_step, _same_state, _same_delay_state = SH.step_all, SH.same_step, SH.same_state, SW.same_side_state
_history, _push = SH.delay_history, SH.push_history


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---- 1. the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,kernel,hist,z,extra", [
    ("quad", "v2", 1, "auto", H2, None, {}),                 # step_kernel_pw, 256-thread form; the history alone
    ("hexa", "v2", 3, "lane", H1, FULL, ALL),                # step_kernel; with everything else on
    ("quad", "v1_raw", 1, "helper", H2, amd.ActionDelay(1, 3), {})])   # step_kernel_pw, 128-thread form; 17 + 8 columns
def test_history_handle_equals_its_twin_and_the_reference_history(vehicle, task, nwp, kernel, hist, z, extra):
    T, H = 60, hist.rows
    a = _env(vehicle, task, nwp, kernel=kernel, action_delay=z, action_history=hist, **extra)
    b = _env(vehicle, task, nwp, kernel=kernel, action_delay=z, **extra)
    base = b.obs_dim
    assert base == (17 if task != "v2" else 20) and a.obs_dim == base + 4 * H == int(a.lib.amenv_obs_dim(a._h)) and int(b.lib.amenv_obs_dim(b._h)) == base
    assert a.kernel_name == b.kernel_name + f" +history {H}" and a.obs.shape == (N, base + 4 * H) == a.terminal_obs.shape
    oa, ob = a.reset().clone(), b.reset().clone()
    assert torch.equal(oa[:, :base], ob) and torch.equal(oa[:, base:], _t(np.tile(HOVER, (N, H)), a.device))
    ref = _history(a, z)
    dev = a.device
    acts = _actions(T + 1, N, 11, dev)
    ended = 0
    for t in range(T):
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, acts[t])
        assert torch.equal(ra[0][:, :base], rb[0]), t
        for x, y in zip(ra[1:4], rb[1:4]):
            assert torch.equal(x, y), t
        assert torch.equal(ra[4][da][:, :base], rb[4][db]) and torch.equal(ra[5][da], rb[5][db]) and torch.equal(ra[6][da], rb[6][db]), t
        _same_state(a, b, t)
        term = history_ref.pushed(ref, acts[t].cpu().numpy(), H)
        reset = _push(ref, a, acts[t], ra[3])
        assert torch.equal(ra[0][:, base:], _t(history_ref.rows(ref, H), dev)), t           # step rows; hover where a new episode started
        assert torch.equal(ra[4][da][:, base:], _t(term, dev)[da]), t                         # terminal rows: the history before the reset
        assert np.array_equal(reset, da.cpu().numpy()), t                                    # (auto-reset: every episode end starts an episode)
        assert np.array_equal(history_ref.rows(ref, H)[reset], np.tile(HOVER, (int(reset.sum()), H)))
        d, recent = a.action_delay_state()
        assert np.array_equal(d.cpu().numpy(), ref.d) and np.array_equal(recent.cpu().numpy().view(np.uint32), ref.recent.view(np.uint32)), t
        if z is not None:
            _same_delay_state(a, b, t)
        ended += int(reset.sum())
    assert ended > N and a.stats() == b.stats()
    if z is None:
        assert not bool(a.action_delay_state()[0].any())
        with pytest.raises(L.AmenvError):
            b.action_delay_state()
    assert torch.equal(a.observe(), a.obs)                                                   # observe(): the last step's row
    mask = torch.zeros(N, dtype=torch.uint8); mask[::3] = 1
    m = mask.numpy() != 0
    cur = history_ref.rows(ref, H)
    oa, ob = a.reset(mask).clone(), b.reset(mask).clone()
    assert torch.equal(oa[:, :base], ob)
    assert torch.equal(oa[:, base:][m], _t(np.tile(HOVER, (int(m.sum()), H)), dev)) and torch.equal(oa[:, base:][~m], _t(cur[~m], dev))
    assert not np.array_equal(cur[~m], np.tile(HOVER, (int((~m).sum()), H)))
    ra, da = _step_all(a, acts[T]); rb, db = _step_all(b, acts[T])                            # and both go on alike
    assert torch.equal(ra[0][:, :base], rb[0]) and torch.equal(ra[1], rb[1])
    _same_state(a, b)
    if "rotor_lag" in extra:
        assert torch.equal(a.rotor_state(), b.rotor_state())
    a.close(); b.close()


# ---- 2. amenv_rollout = steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,task,nwp,hist,z", [("quad", "v2", 1, H2, None), ("hexa", "v2", 3, H1, FULL), ("quad", "v1_raw", 1, H2, FULL)])
def test_history_rollout_equals_steps(vehicle, task, nwp, hist, z):
    T = 30
    a = _env(vehicle, task, nwp, action_delay=z, action_history=hist)
    b = _env(vehicle, task, nwp, action_delay=z, action_history=hist)
    ro = SH.check_rollout_equals_steps(a, b, _actions(T, N, 2, a.device), min_ended=N // 2, side=(SW,))
    assert ro["obs"].shape == (T, N, a.obs_dim)
    a.close(); b.close()


# ---- 3., 4. the closed loop replays through amenv_step -----------------------------------------------------------------------------
def _closed_loop_replay(vehicle, task, nwp, n, T, hist, z, steps_max):
    env = _env(vehicle, task, nwp, n=n, action_delay=z, action_history=hist, max_episode_steps=steps_max)
    ref = _env(vehicle, task, nwp, n=n, kernel="lane", action_delay=z, action_history=hist, max_episode_steps=steps_max)
    assert env.kernel_name.endswith(f" +history {hist.rows}")
    base = env.obs_dim - 4 * hist.rows
    row0 = None

    def start(env, ref):
        nonlocal row0
        warm = _actions(3, n, 8, env.device)
        for t in range(3):                               # a start state with rows in the history
            env.step(warm[t])
        ref.set_state(*env.get_state())
        ref.set_action_delay_state(*env.action_delay_state())
        row0 = env.observe()
        assert torch.equal(row0[:, base:base + 4], warm[2]) or bool(env.done.any())

    def given_row(t, given, o, r, d, i):
        keep = ~d.bool()
        assert torch.equal(o[keep][:, base:base + 4], given[keep]), t          # the clipped sample is the given row

    run = SH.check_closed_loop_replays(env, ref, T, fill=float("nan"), side=(SW,), prepare=start, each_step=given_row, totals=False)
    assert torch.equal(run.b["obs"][0], row0)            # row 0: the current history
    run.close()


@pytest.mark.parametrize("z", [None, amd.ActionDelay(0, 2)])
def test_history_closed_loop_200_envs_replays_bit_for_bit(z):
    """16-env workgroups.  A quadrotor on the single-waypoint v2 task is a config the lane-quad closed loop would serve: with the history on
    it runs the one-lane-per-env form, whose rows the lane step kernel reproduces."""
    _closed_loop_replay("quad", "v2", 1, N, 40, H2, z, 25)


@pytest.mark.parametrize("vehicle,task,nwp,n,hist", [("hexa", "v2", 2, 6209, H2), ("quad", "v1_raw", 1, 24641, H1)])
def test_history_closed_loop_larger_workgroups(vehicle, task, nwp, n, hist):
    """64-env workgroups (6145..24576 envs) and 128-env workgroups (above), both ragged; episodes of 4 steps end inside the 6."""
    _closed_loop_replay(vehicle, task, nwp, n, 6, hist, amd.ActionDelay(0, 2), 4)


# ---- 5. the MLP reads the new columns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,od", [("v2", 28), ("v1_raw", 25)])
def test_history_rollout_mlp_vs_bf16_model(task, od):
    """test_rollout_mlp_vs_bf16_model's gate on the wider rows: the kernel's mean (raw - exp(log_std) z_fp64) and value against
    forward_bf16_model(two_part=True) on the published rows.  median <= 1e-5, 99.9 % <= 5e-4, max <= 5e-3, fp64 < 3e-2 of the column's scale."""
    T, n, seed, draw0 = 24, 300, 93, 5
    env = _env("quad", task, 1, n=n, max_episode_steps=60, action_history=H2)
    assert env.obs_dim == od
    pol = nondegenerate_policy(od, 4, seed=od + 4, device="cuda")
    env.reset()
    warm = _actions(2, n, 3, env.device)
    for t in range(2):
        env.step(warm[t])
    b = _nan_buffers(T, n, od, env.device)
    env.rollout_policy(pol.flat_param, T, seed, draw0, **b)
    torch.cuda.synchronize()
    SH.all_written(b)
    hist_cols = b["obs"][:T, :, od - 8:]
    assert float(hist_cols.std()) > 0.3                    # the history columns carry the (order-one) actions
    zr = torch.from_numpy(philox_normals_fp64(seed, GID0 + np.arange(n)[None, :], (draw0 + np.arange(T))[:, None], 4)).to(env.device)
    mean_k = (b["actions"].double() - torch.exp(pol.log_std.detach().double()) * zr).reshape(T * n, 4)
    val_k = b["values"].double().reshape(-1)
    obs = b["obs"][:T].reshape(T * n, od)
    m_ref, v_ref = forward_bf16_model(pol, obs, True)
    m64, v64 = forward_fp64(pol, obs)
    cols = [(f"mean[{k}]", mean_k[:, k], m_ref[:, k], m64[:, k]) for k in range(4)] + [("value", val_k, v_ref, v64)]
    report, fails = [], []
    for name, got, ref, r64 in cols:
        scale = max(1.0, float(ref.abs().max()))
        e = (got - ref).abs() / scale
        q50, q999, mx = float(e.median()), float(e.quantile(0.999)), float(e.max())
        e64 = float((got - r64).abs().max()) / scale
        report.append(f"{name} {q50:.1e}/{q999:.1e}/{mx:.1e} fp64 {e64:.1e}")
        if not (q50 <= 1e-5 and q999 <= 5e-4 and mx <= 5e-3 and e64 < 3e-2):
            fails.append((name, q50, q999, mx, e64))
    print(f"\n[history MLP] od {od}: |kernel - bf16 model| / scale median / 99.9% / max: " + "; ".join(report))
    assert not fails, fails
    env.close()


# ---- 6. the fp32-grade kernels at the new shapes -------------------------------------------------------------------------------------
SHAPES = [(24, 4), (28, 4), (21, 4), (25, 4)]


@pytest.mark.parametrize("D,A,n", [(D, A, n) for D, A in SHAPES for n in (1, 1000, 32768) if n < 32768 or D == 28])
def test_forward_kernels_vs_fp64_new_shapes(D, A, n):
    """amenv_policy_forward (VALU) and amenv_policy_forward_mfma within 2e-5 of the scale of forward_fp64 (test_forward_kernels_vs_fp64's gate)."""
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
        print(f"({D},{A}) n {n} {form}: mean {em:.2e} value {ev:.2e}")
        assert em < 2e-5 and ev < 2e-5, (form, em, ev)


@pytest.mark.parametrize("D,A", SHAPES)
def test_fused_mlp_step_vs_fp64_autograd_new_shapes(D, A):
    """amenv_ppo_mlp_step against the same loss differentiated in fp64 (test_fused_mlp_step_vs_fp64_autograd's bars): the error is at most
    max(4 x torch fp32's, 2e-6) of the largest entry, and every parameter block on its own at most max(4 x torch fp32's error in that
    block, 1e-5 x the block's largest entry)."""
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
    print(f"\n({D},{A}) n {n}: gradient error vs fp64 autograd / largest entry: torch fp32 {e_torch:.2e}, fused kernel {e_fused:.2e}")
    assert e_fused < max(4.0 * e_torch, 2e-6), (e_fused, e_torch)
    assert 0.02 < float(s[3]) < 0.9                                         # clip fraction: both branches of the clipped objective ran
    off = 0
    for name, p_ in pol.named_parameters():
        k = p_.numel()
        blk = float(g64[off:off + k].abs().max())
        et = float((grads[False][off:off + k] - g64[off:off + k]).abs().max())
        ef = float((grads[True][off:off + k] - g64[off:off + k]).abs().max())
        assert blk > 0 and ef <= max(4.0 * et, 1e-5 * blk), (name, ef, et, blk)
        off += k


# ---- 7. toggling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [None, FULL])
def test_history_set_and_cleared_is_bit_invisible(z):
    a = _env("hexa", "v2", 2, action_delay=z)
    b = _env("hexa", "v2", 2, action_delay=z)
    base, name = b.obs_dim, b.kernel_name
    assert torch.equal(a.reset(), b.reset())
    acts = _actions(18, N, 6, a.device)
    for t in range(5):
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, acts[t])
    a.set_action_history(H2)
    assert a.obs_dim == base + 8 and a.kernel_name == name + " +history 2" and a.action_history is H2
    for t in range(5, 8):                                # while it is on: the task's columns and everything else are the twin's
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, acts[t])
        assert torch.equal(ra[0][:, :base], rb[0]) and torch.equal(ra[0][~da][:, base:base + 4], acts[t][~da]), t
    a.set_action_history(None)
    assert a.obs_dim == base == int(a.lib.amenv_obs_dim(a._h)) and a.kernel_name == name and a.action_history is None and a.obs.shape == (N, base)
    for t in range(8, 18):
        ra, da = _step_all(a, acts[t]); rb, db = _step_all(b, acts[t])
        _same_step(ra, da, rb, db, t)
        _same_state(a, b, t)
        if z is not None:
            _same_delay_state(a, b, t)
    assert a.stats() == b.stats()
    a.close(); b.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
_wide_row = functools.partial(SH.one_action, rows=_actions)


def test_history_refusals_leave_everything_untouched():
    def on(env):
        od = env.obs_dim
        with pytest.raises(L.AmenvError):
            env.set_action_history(H2)
        assert env.obs_dim == od == int(env.lib.amenv_obs_dim(env._h))

    def bad_rows(env):     # rows outside 0..2, past the Python class
        for rows in (3, -1):
            assert env.lib.amenv_set_action_history(env._h, rows) == -1 and b"rows" in env.lib.amenv_last_error(env._h), rows
        assert int(env.lib.amenv_obs_dim(env._h)) == 20 and "+history" not in env.lib.amenv_kernel_name(env._h).decode()

    refused = functools.partial(SH.check_refused, SW, action=_wide_row)
    refused(lambda: _env("hexa_arm", n=64), on)
    refused(lambda: _env(n=64, dtype="f64"), on)
    refused(lambda: _env(n=64, kernel="team"), on)
    refused(lambda: amd.GpuWaypointEnv(64, config=SH.octo_config(64, GID0)), on)
    refused(lambda: _env(n=64), bad_rows)
    # the normaliser inside the launch, while the history is on
    env, twin = _env(n=64, action_history=H2), _env(n=64, action_history=H2)
    env.reset(); twin.reset()
    od, dev = env.obs_dim, env.device
    nrm = ObsNormalizer(od)
    nrm.update(env.observe())
    before = nrm.get()
    b = _nan_buffers(4, 64, od, dev)
    with pytest.raises(L.AmenvError, match="history"):
        env.rollout_policy(SH.policy(od).flat_param, 4, seed=1, draw0=0, obs_normalizer=nrm, **b)
    torch.cuda.synchronize()
    assert bool(torch.isnan(b["obs"]).all())
    for x, y in zip(before, nrm.get()):
        assert np.array_equal(x, y)
    SH.next_step_alike(env, twin, _wide_row)
    _same_delay_state(env, twin)
    nrm.close(); env.close(); twin.close()


# ---- 9. sharding and restore -------------------------------------------------------------------------------------------------------
def test_history_two_shards_equal_one_handle_and_restore():
    n, T, cut = 200, 40, 100
    kw = dict(seed=13, max_episode_steps=20, action_delay=FULL, action_history=H2)
    whole = _env("hexa", "v2", 1, n=n, **kw)
    h0 = _env("hexa", "v2", 1, n=cut, **kw)
    h1 = _env("hexa", "v2", 1, n=n - cut, env_id_offset=GID0 + cut, **kw)
    acts = _actions(T + 10, n, 4, whole.device)
    SH.check_two_shards(whole, h0, h1, cut, acts[:T], side=(SW,))
    # restore into a fresh handle: get_state + action_delay_state are the whole state
    fresh = _env("hexa", "v2", 1, n=n, **kw)
    fresh.reset()
    fresh.set_state(*whole.get_state())
    fresh.set_action_delay_state(*whole.action_delay_state())
    assert torch.equal(fresh.observe(), whole.obs)
    for t in range(T, T + 10):
        ra, da = _step_all(whole, acts[t]); rb, db = _step_all(fresh, acts[t])
        _same_step(ra, da, rb, db, t)
    _same_state(whole, fresh)
    _same_delay_state(whole, fresh)
    for e in (whole, h0, h1, fresh):
        e.close()


# ---- 10. host side -----------------------------------------------------------------------------------------------------------------
def test_history_host_side_integration():
    n = 64
    env = _env(n=n, action_history=H2)
    assert env.obs_dim == 28
    obs = env.reset()
    nrm = ObsNormalizer(env.obs_dim)
    acts = _actions(12, n, 5, env.device)
    seen = [obs.clone()]
    nrm.update(obs)
    for t in range(12):
        obs, _, _, _ = env.step(acts[t])
        nrm.update(obs)
        seen.append(obs.clone())
    rows = torch.cat(seen).double()
    mean, var = (torch.as_tensor(x).double().cpu() for x in nrm.get()[:2])
    # fp64 running moments of all 28 columns; the normaliser's prior (count 1e-4, mean 0, var 1) against 832 rows moves them by < 1e-6
    assert mean.shape == (28,) and torch.allclose(mean, rows.mean(0).cpu(), rtol=0, atol=1e-6)
    assert torch.allclose(var, rows.var(0, unbiased=False).cpu(), rtol=0, atol=1e-6) and bool((var[20:] > 1e-3).all())
    out = nrm.normalize(obs)
    want = ((obs.double() - mean.to(obs.device)) / torch.sqrt(var.to(obs.device) + nrm.epsilon)).clamp(-nrm.clip_obs, nrm.clip_obs)
    assert out.shape == (n, 28) and torch.allclose(out.double(), want, rtol=0, atol=2e-6)                # (one fp32 rounding of values up to clip_obs = 10: an ulp is 9.5e-7)
    nrm.close()
    algo = PPO(env, n_steps=16, batch_size=1024, fused_rollout=True, seed=1)
    assert algo.policy.obs_dim == 28
    algo.learn(2 * 16 * n)
    assert len(algo.log) == 2 and all(math.isfinite(x) for rec in algo.log for x in rec.values())
    assert algo.buffer.obs.shape[-1] == 28 and bool((algo.buffer.obs[1:, :, 20:24] != 1.0).any())
    nrm2 = ObsNormalizer(env.obs_dim)
    with pytest.raises(L.AmenvError, match="step-by-step"):
        PPO(env, n_steps=16, batch_size=1024, obs_normalizer=nrm2, fused_rollout=True)
    step_by_step = PPO(env, n_steps=16, batch_size=1024, obs_normalizer=nrm2, fused_rollout=False, seed=1)
    step_by_step.learn(16 * n)
    assert len(step_by_step.log) == 1
    nrm2.close(); env.close()
    vec = amd.GpuVecEnv(num_envs=64, action_history=amd.ActionHistory(2))
    assert vec.observation_space.shape == (28,) and vec.reset().shape == (64, 28)
    vec.close()


# ---- 11. independent of the twin: the unchanged fp64 oracle --------------------------------------------------------------------------
def test_history_kernel_matches_the_history_oracle():
    """fp32 quadrotor with the delay and two rows of history against history_ref.HistoryOracle, teacher-forced per step, under
    test_delayed_kernel_matches_the_delayed_oracle's gate: state and the task's columns within 1e-5 max(1, |x|), flag bits equal except at
    most one threshold flip in 16,000 env-steps.  The history columns are compared exactly."""
    T, H = 80, 2
    env = _env(action_delay=FULL, action_history=H2, seed=5)
    cfg = O.reference_quad_config(num_envs=N, seed=5)
    cfg.task.max_episode_steps = 25
    cfg.env_id_offset = GID0
    orc = history_ref.HistoryOracle(cfg, H, 0, 8)
    o0 = env.reset().cpu().numpy(); r0 = orc.reset()
    assert np.array_equal(o0[:, 20:], r0[:, 20:].astype(np.float32)) and np.array_equal(env.action_delay_state()[0].cpu().numpy(), orc.hist.d)
    acts = _actions(T, N, 21, env.device)
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
        if nd.any():
            err = np.abs(f[:13][:, nd] - orc.env.fstate[:13][:, nd]) / np.maximum(1.0, np.abs(orc.env.fstate[:13][:, nd]))
            worst = max(worst, float(err.max()))
        g = obs.cpu().numpy()
        eo = np.abs(g[ok, :20].astype(np.float64) - o["obs"][ok, :20]) / np.maximum(1.0, np.abs(o["obs"][ok, :20]))
        worst_o = max(worst_o, float(eo.max()))
        assert np.array_equal(g[ok, 20:], o["obs"][ok, 20:].astype(np.float32)), t
        gt = env.terminal_obs.cpu().numpy()
        assert np.array_equal(gt[dn, 20:], o["terminal_hist"][dn]), t
        d, recent = (x.cpu().numpy() for x in env.action_delay_state())
        for j in np.flatnonzero(bad):     # a flipped env: the oracle's history follows the GPU's episode
            orc.hist.d[j] = d[j]; orc.hist.recent[j] = recent[j]
    print(f"history vs oracle: state {worst:.3e} obs {worst_o:.3e} flips {flips} episode ends {dones}")
    assert worst <= 1e-5 and worst_o <= 1e-5, (worst, worst_o)
    assert flips <= 1 and dones > N
    env.close()
