"""amenv_pid_policy (pid_policy_kernel, csrc/amenv_baseline.hpp) and amenv_minsnap_eval against independent references on the MI355X.

The PID policy is compared with tests/pid_policy_ref.py (plain numpy, fp64, pinned on the CPU by tests/test_pid_policy_ref_cpu.py) in
every product configuration: rigid vehicles and 1- / 2- / 3-link arms, tool and base task points, in-episode waypoint switches, an
observation row that is not 20 / 25 / 27 / 29 wide, ragged and single-row launches, the restart contract, the refusals, and the fp32
build (the one that flies and that PPO clones) against the fp64 reference with the numpy restatement run in float32 as the yardstick.
The trajectory evaluation is compared with MinSnapTrajectory's torch path off the recorded helix: many trajectories, gathers, knots, ends."""
import ctypes as C

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.baselines import MinSnapTrajectory, PidWaypointPolicy
from tests import pid_policy_ref as R

pytestmark = pytest.mark.gpu
ULP1 = float(np.spacing(np.float32(1.0)))     # one fp32 ulp of an action of size 1: the floor of every action comparison


def gpu_env(s, n=None):
    return amd.GpuWaypointEnv(s["n"] if n is None else n, vehicle=s["vehicle"], seed=R.SEED, num_waypoints=s["K"], n_joints=s["n_joints"],
                              ee_task=s["ee_task"], max_episode_steps=s["limit"], action_history=amd.ActionHistory(s["history"]) if s["history"] else None)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def params_of(pol, width, **over):
    """The C ABI's parameter block as PidWaypointPolicy builds it for rows `width` wide, with fields overridden."""
    p = L.PidPolicyParams(pid=pol.pid.params(), speed=pol.speed, moment_scale=pol.moment_scale, obs_dim=width, act_dim=pol.act_dim,
                          tool_mode=int(pol.tool_mode))
    p.inertia_ratio[:] = pol.inertia_ratio
    for k, v in over.items():
        setattr(p, k, v)
    return p


def launch(p, dtype_code, obs, done, pstate, act, n):
    rc = L.load().amenv_pid_policy(C.byref(p), dtype_code, ptr(obs), ptr(done), ptr(pstate), ptr(act), n,
                                   C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    torch.cuda.synchronize()
    return rc


def action_tol(b):
    """One fp32 ulp of max(1, |a|): both sides do the same fp64 operations on the same fp32 inputs and round to fp32 once."""
    return np.spacing(np.maximum(1.0, np.abs(b)).astype(np.float32)).astype(np.float64)


def arm_policy_pair(n, dtype, tool_mode=True):
    """A HIP policy and the reference for n synthetic 29-wide rows of the default 3-link arm (no env behind them)."""
    cfg = L.default_config("hexa_arm", n)
    v = cfg.vehicle
    pol = PidWaypointPolicy(n, dt=cfg.task.dt, mass=v.mass, g=v.g, moment_scale=v.moment_scale, inertia_diag=(v.inertia[0], v.inertia[4], v.inertia[8]),
                            speed=R.SPEED, device="cuda", dtype=dtype, act_dim=7, tool_mode=tool_mode)
    ref = R.PidPolicyRef.for_config(cfg, 29, 7, speed=R.SPEED)
    ref.tool_mode = tool_mode
    return pol, ref


def synthetic_rows(rng, rows, obs_dim):
    o = rng.normal(size=(rows, obs_dim)) * 0.1
    o[:, 6:10] = rng.normal(size=(rows, 4)) * 0.15 + np.array([1.0, 0.0, 0.0, 0.0])     # near level, not unit length
    o[:, 13:16] = rng.normal(size=(rows, 3)) * 0.3
    return o.astype(np.float32)


# ---- fp64 build against the reference, closed loop ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.STREAMS))
def test_fp64_build_equals_the_reference_on_every_call(name):
    s = R.STREAMS[name]
    env = gpu_env(s)
    n = s["n"]
    hip = PidWaypointPolicy.for_env(env, speed=R.SPEED, dtype=torch.float64)
    ref = R.PidPolicyRef.for_config(env.cfg, env.obs_dim, env.act_dim, speed=R.SPEED)
    assert hip.pstate is not None and hip.pstate.dtype == torch.float64
    assert hip.tool_mode == ref.tool_mode == (s["ee_task"] == "tool") and hip.act_dim == env.act_dim == ref.act_dim
    assert env.obs_dim == {None: 20, 1: 25, 2: 27, 3: 29}[s["n_joints"]] + 4 * s["history"]
    obs, done, ends, worst = env.reset(), None, 0, 0.0
    for _ in range(s["steps"]):
        a = hip.predict(obs, done)
        b = ref.predict(obs.cpu().numpy(), None if done is None else done.cpu().numpy())
        an = a.cpu().numpy()
        err = np.abs(an.astype(np.float64) - b.astype(np.float64))
        worst = max(worst, float(err.max()))
        assert np.all(err <= action_tol(b)), (name, float(err.max()))
        assert an.shape == (n, env.act_dim) and np.all(an[:, 4:] == 0.0)
        obs, _, done, _ = env.step(a)
        ends += int(done.sum())
    print(f"{name}: worst action difference {worst:.3e}, ends {ends}, switches {ref.switches}, fresh starts {ref.fresh_starts}")
    np.testing.assert_allclose(hip.pstate.cpu().numpy(), ref.state, rtol=1e-9, atol=1e-12)
    assert ends >= R.ends_floor(s) and ref.switches >= R.switches_floor(s)
    assert ref.fresh_starts == n + ends - int(done.sum())     # every episode start but the ones the last step left pending
    env.close()


# ---- launch geometry: nothing past n ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_rows_past_n_are_not_written(n, dtype):
    """The launcher rounds the grid up to 64-lane blocks: lanes n.. must return before they load or store.  Every buffer carries 64 more
    rows than the call is told about; afterwards those rows of `actions` and `pstate` hold their sentinel bits."""
    pad, rng = 64, np.random.RandomState(n)
    pol, ref = arm_policy_pair(n, dtype)
    p = params_of(pol, 29)
    pst = torch.full((n + pad, 14), 123.0, device="cuda", dtype=dtype)
    pst[:n] = pol.pstate
    act = torch.full((n + pad, 7), -7.25, device="cuda", dtype=torch.float32)
    pst0, act0 = pst.clone(), act.clone()
    ints = torch.int64 if dtype == torch.float64 else torch.int32
    for call in range(2):
        o = synthetic_rows(rng, n + pad, 29)
        d = (rng.uniform(size=n + pad) < 0.3).astype(np.uint8)
        d[n:] = 1                                   # a lane past n that ran would restart its row: t = dt, a visible write
        done = None if call == 0 else torch.from_numpy(d).cuda()
        assert launch(p, L.F64 if dtype == torch.float64 else L.F32, torch.from_numpy(o).cuda(), done, pst, act, n) == 0
        assert torch.equal(pst[n:].view(ints), pst0[n:].view(ints)) and torch.equal(act[n:].view(torch.int32), act0[n:].view(torch.int32))
        b = ref.predict(o[:n], None if call == 0 else d[:n])
        a = act[:n].cpu().numpy()
        assert np.all(a[:, 4:] == 0.0) and float(pst[:n, 13].abs().max()) == 0.0
        if dtype == torch.float64:
            assert np.all(np.abs(a.astype(np.float64) - b) <= action_tol(b))
            np.testing.assert_allclose(pst[:n].cpu().numpy(), ref.state, rtol=1e-9, atol=1e-12)


# ---- the restart contract ----------------------------------------------------------------------------------------------------------------

def test_restart_contract():
    s = R.STREAMS["arm2_tool"]
    n = 130
    env = gpu_env(s, n=n)
    A = PidWaypointPolicy.for_env(env, speed=R.SPEED, dtype=torch.float64)
    ref = R.PidPolicyRef.for_config(env.cfg, env.obs_dim, env.act_dim, speed=R.SPEED)
    obs = env.reset()
    # (1) the first call, done = None: every row starts from its fresh flag, and the flag is cleared
    assert float(A.pstate[:, 13].min()) == 1.0
    a = A.predict(obs, None)
    ref.predict(obs.cpu().numpy(), None)
    st = A.pstate.cpu().numpy()
    o64 = obs.cpu().numpy().astype(np.float64)
    point = o64[:, 0:3] * 10.0 + o64[:, -3:] * 0.5
    assert np.all(st[:, 13] == 0.0) and np.all(st[:, 0] == env.cfg.task.dt) and ref.fresh_starts == n
    assert np.array_equal(st[:, 1:4], point) and np.array_equal(st[:, 4:7], point + o64[:, 13:16] * 2.0)
    np.testing.assert_allclose(st, ref.state, rtol=1e-9, atol=1e-12)
    for _ in range(25):
        obs, _, _, _ = env.step(a)
        a = A.predict(obs, None)
    obs, _, _, _ = env.step(a)
    # (2) a done mask restarts exactly the flagged rows; every other row is the run without a mask
    before = A.pstate.clone()
    assert float(before[:, 0].median()) > 20 * env.cfg.task.dt and float(before[:, 7:13].abs().max()) > 0.0
    mask = torch.zeros(n, dtype=torch.uint8, device=obs.device)
    mask[torch.from_numpy(np.random.RandomState(0).permutation(n)[:n // 3].copy()).to(obs.device)] = 1
    m = mask.bool()
    a_mask = A.predict(obs, mask)
    st_mask = A.pstate.clone()
    A.pstate.copy_(before)
    a_none = A.predict(obs, None)
    st_none = A.pstate.clone()
    A.pstate.zero_()
    A.pstate[:, 13] = 1.0
    a_new = A.predict(obs, None)                    # one step from zero: a new episode on the same rows
    st_new = A.pstate.clone()
    assert torch.equal(a_mask[~m], a_none[~m]) and torch.equal(st_mask[~m], st_none[~m])
    assert torch.equal(a_mask[m], a_new[m]) and torch.equal(st_mask[m], st_new[m])
    assert not torch.equal(a_mask[m], a_none[m]) and float(st_none[:, 0].median()) > 20 * env.cfg.task.dt
    o64 = obs.cpu().numpy().astype(np.float64)
    point = o64[:, 0:3] * 10.0 + o64[:, -3:] * 0.5
    mm = m.cpu().numpy()
    stm = st_mask.cpu().numpy()
    assert np.all(stm[mm, 0] == env.cfg.task.dt) and np.array_equal(stm[mm, 1:4], point[mm]) and np.all(stm[:, 13] == 0.0)
    # (3) predict() takes a bool or a strided mask for the same result
    for other in (m, torch.stack([mask, 1 - mask], 1)[:, 0], mask.to(torch.int64)):
        assert other.dtype != torch.uint8 or not other.is_contiguous()
        A.pstate.copy_(before)
        assert torch.equal(A.predict(obs, other), a_mask) and torch.equal(A.pstate, st_mask)
    env.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,over,n,dtype_code", [
    ("obs_dim 19", dict(obs_dim=19), 64, L.F64), ("tool mode, obs_dim 22", dict(obs_dim=22, tool_mode=1), 64, L.F64),
    ("act_dim 3", dict(act_dim=3), 64, L.F64), ("act_dim 17", dict(act_dim=17), 64, L.F64), ("speed 0", dict(speed=0.0), 64, L.F64),
    ("moment_scale 0", dict(moment_scale=0.0), 64, L.F64), ("n 0", {}, 0, L.F64), ("dtype 2", {}, 64, 2)])
def test_refusals_return_minus_one_and_write_nothing(case, over, n, dtype_code):
    pol, _ = arm_policy_pair(64, torch.float64, tool_mode=False)
    p = params_of(pol, 29, **over)
    obs = torch.from_numpy(synthetic_rows(np.random.RandomState(1), 64, 32)).cuda()
    pst = torch.full((64, 14), 123.0, device="cuda", dtype=torch.float64)
    pst[:, 13] = 1.0
    act = torch.full((64, 32), -7.25, device="cuda", dtype=torch.float32)
    pst0, act0 = pst.clone(), act.clone()
    assert launch(p, dtype_code, obs, None, pst, act, n) == -1, case
    assert torch.equal(pst.view(torch.int64), pst0.view(torch.int64)) and torch.equal(act.view(torch.int32), act0.view(torch.int32)), case
    assert launch(params_of(pol, 29), L.F64, obs[:, :29].contiguous(), None, pst, act, 64) == 0      # the same buffers are accepted otherwise
    assert not torch.equal(act, act0)


# ---- fp32 build against the fp64 reference ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["quad_k3", "arm1_tool", "arm3_tool"])
def test_fp32_build_is_as_close_to_fp64_as_the_same_formulae_in_float32(name):
    """Teacher-forced: before each call the fp32 state block is the fp32 cast of the reference's fp64 state, so each call is one evaluation.
    Yardstick = the numpy restatement in float32 on the same rows and state (never the kernel).  Per action column the kernel's median and
    99th percentile of |a32 - a64| may be at most 4 x the yardstick's (same formulae, same precision; what differs is libm's asinf /
    atan2f / sqrtf and the rounding of divisions), with one fp32 ulp of an action as the floor of both; the share of rows above 1e-3 at
    most the yardstick's + 1 percentage point.  The per-row maximum is not bounded: the moment vector is multiplied by the inertia ratio
    and normalised by its largest component, and the fp64-vs-float32 restatement alone reaches 0.48 on the 3-link arm."""
    s = R.STREAMS[name]
    env = gpu_env(s)
    hip = PidWaypointPolicy.for_env(env, speed=R.SPEED)
    assert hip.pstate.dtype == torch.float32
    r64 = R.PidPolicyRef.for_config(env.cfg, env.obs_dim, env.act_dim, speed=R.SPEED)
    y32 = R.PidPolicyRef.for_config(env.cfg, env.obs_dim, env.act_dim, speed=R.SPEED, dtype=np.float32)
    obs, done, ek, ey, ends = env.reset(), None, [], [], 0
    for _ in range(300):
        st32 = r64.state.astype(np.float32)
        hip.pstate.copy_(torch.from_numpy(st32))
        y32.state = st32.copy()
        on, dn = obs.cpu().numpy(), None if done is None else done.cpu().numpy()
        a = hip.predict(obs, done)
        a64 = r64.predict(on, dn).astype(np.float64)
        ek.append(np.abs(a.cpu().numpy()[:, :4] - a64[:, :4]))
        ey.append(np.abs(y32.predict(on, dn)[:, :4] - a64[:, :4]))
        obs, _, done, _ = env.step(a)
        ends += int(done.sum())
    ek, ey = np.concatenate(ek), np.concatenate(ey)
    q = lambda e: np.percentile(e, [50, 99], axis=0)          # noqa: E731  -> [2, 4]
    qk, qy = q(ek), q(ey)
    share_k, share_y = float((ek.max(1) > 1e-3).mean()), float((ey.max(1) > 1e-3).mean())
    with np.printoptions(precision=2):
        print(f"{name}: {ek.shape[0]} rows, ends {ends}, switches {r64.switches}")
        print(f"  kernel    median {qk[0]}  p99 {qk[1]}  rows > 1e-3: {share_k:.4%}  (max {ek.max():.2e})")
        print(f"  yardstick median {qy[0]}  p99 {qy[1]}  rows > 1e-3: {share_y:.4%}  (max {ey.max():.2e})")
    assert np.all(qk <= 4.0 * np.maximum(qy, ULP1)), (qk, qy)
    assert share_k <= share_y + 0.01
    assert r64.switches >= R.switches_floor(s) and ends >= R.ends_floor(s)
    env.close()


# ---- amenv_minsnap_eval off the recording ------------------------------------------------------------------------------------------------

def _query_times(rng, S, traj, n):
    """Times for queries on trajectories `traj`, cycling through: exactly 0, every inner knot, exactly the end, past the end, interior."""
    t, kind = np.zeros(len(traj)), np.zeros(len(traj), np.int64)
    for i, b in enumerate(traj):
        c = (i + int(rng.randint(0, n + 4)) * (len(traj) == 1)) % (n + 4)
        kind[i] = c
        end = S[b, n]
        t[i] = 0.0 if c == 0 else S[b, c] if c < n else end if c == n else 1.5 * end if c == n + 1 else rng.uniform(0.0, end)
    return t, kind


@pytest.mark.parametrize("n", [1, 2, 7, 16])
def test_min_snap_eval_kernel_on_many_trajectories(n):
    B, rng = 33, np.random.RandomState(5 + n)
    w = rng.uniform(-3, 3, size=(B, n + 1, 3))
    dev, cpu = MinSnapTrajectory(torch.from_numpy(w).cuda(), 0.9), MinSnapTrajectory(torch.from_numpy(w), 0.9)
    # MST matches derivatives 1..6 at an inner knot in each segment's own scaled time, so velocity and acceleration per second jump there
    # wherever the neighbours' durations differ: "exactly on knot k" selects a segment, and only means something against ONE table of knot
    # times.  The device's and torch's tables agree to rtol 1e-14 (the solve test's bound) but not in every last bit (the norm sums in
    # another order), so both sides evaluate on the device's table; the coefficients stay each side's own (Gauss-Jordan vs linalg.solve).
    assert torch.allclose(dev.T.cpu(), cpu.T, rtol=1e-14, atol=0) and torch.allclose(dev.S.cpu(), cpu.S, rtol=1e-14, atol=1e-15)
    print(f"n={n}: {int((dev.S.cpu() != cpu.S).sum())} of {cpu.S.numel()} knot times differ in their last bits between device and torch")
    cpu.T, cpu.S = dev.T.cpu(), dev.S.cpu()
    S = cpu.S.numpy()                                         # the knots the kernel compares with
    scale = max(1.0, float(cpu.coeff.abs().max()))
    queries = [(None, np.arange(B))] + [("gather", np.concatenate([rng.permutation(B) for _ in range(m // B + 1)])[:m]) for m in (1, 257, 1200)]
    for how, traj in queries:
        t, kind = _query_times(rng, S, traj, n)
        tt = torch.from_numpy(t)
        ti = None if how is None else torch.from_numpy(traj)
        des = dev.evaluate(tt.cuda(), traj=None if ti is None else ti.cuda()).cpu().numpy()
        want = cpu.evaluate(tt, traj=ti).numpy()
        assert des.shape == (len(traj), 11) and len(traj) in (1, 33, 257, 1200)
        e = np.abs(des - want)
        print(f"n={n} m={len(traj)} {how}: pos {e[:, 0:3].max():.2e} vel {e[:, 3:6].max():.2e} acc {e[:, 6:9].max():.2e} (x {scale:.3g})")
        assert e[:, 0:3].max() < 1e-11 * scale and e[:, 3:6].max() < 1e-11 * scale and e[:, 6:9].max() < 1e-10 * scale
        assert np.all(des[:, 9:11] == 0.0)
        if len(traj) > 1:
            assert set(kind) == set(range(n + 4))             # every kind of time was asked
        first, after = kind == 0, kind == n + 1
        assert np.array_equal(des[first, 0:3], w[traj[first], 0]) and np.array_equal(des[after, 0:3], w[traj[after], n])
        assert np.all(des[first | after, 3:9] == 0.0)
        d32 = dev.evaluate(tt.cuda(), traj=None if ti is None else ti.cuda(), dtype=torch.float32).cpu().numpy()
        assert d32.dtype == np.float32 and np.abs(d32 - des).max() < 2e-6 * max(1.0, np.abs(des).max())
