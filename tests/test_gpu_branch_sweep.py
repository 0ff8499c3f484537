"""Every step-kernel family on every branch of the step state machine, against the fp64 oracle (`pytest -m gpu`).

The state machine (`task_step`, csrc/amenv_model.hpp) is one piece of code, but each family feeds it and publishes its results through plumbing of
its own (DPP broadcasts and an episode-end helper wave in the lane-team kernel, LDS hand-overs in the stage-wave, two-wave, lane-quad and
helper-wave kernels, the inline episode-end path in the rollout kernels).  Here each family starts from the blob of tests/state_blob.py -- envs
in the hold phase with counters on both sides of counter_limit, first arrivals, crashes sinking and rising, out of bounds, the time limit,
both signs of the progress bonus -- and every output of six teacher-forced steps is compared with the oracle's by `state_blob.compare`
(gates in that file's docstring); then amenv_rollout and amenv_rollout_policy from the same states against amenv_step, bit for bit.

The kernels are built in three compile-time task forms, and the sweep runs all three:
  VAR_V2, KW=1   one waypoint (SWEEP: every family)
  VAR_V1, KW=2   v1_raw / v1_scaled (TASK_SWEEP): `task_step_v1` -- the waypoint count per episode in flag bits 4-7, +-10 approach shaping, a
                 final reach that returns before the step counter moves and before the time-limit test, the is_final column, what the reset drew
  VAR_V2, KW=4   2..4 waypoints (TASK_SWEEP), rigid vehicles and the arm: an intermediate reach that falls through to the crash and
                 out-of-bounds tests, the next-waypoint columns, last_distance across a switch, the hold phase at index K
On the last two the rigid helper-wave kernel is its 128-thread form (the main wave forms the rows, draws the next episode and writes the Monitor
rows and totals itself) and the arm runs its KW=4 lane kernel; the families built for one waypoint only must refuse these tasks.
Worst errors measured on the TASK_SWEEP cases (MI355X, 12 cases x 6 steps x 300 envs, 0 threshold flips), v1 / several waypoints:
  fp32: state 4.6e-6 / 4.8e-6, reward 5.2e-6 / 6.1e-6, observation rows 2.4e-7 / 1.8e-7, ep_return 1.2e-6 / 1.8e-6, terminal rows 1.2e-7 / 1.2e-7
  fp64: state 4.3e-14 / 1.1e-13, reward 7.2e-15 / 1.3e-14, observation rows 6.6e-17 / 1.3e-17, ep_return 0 / 0, terminal rows 0 / 0

tests/test_state_blob_cpu.py checks on the oracle alone that these states reach every branch and that the envs a flip could be excused on
number no more than the cap.  tests/test_gpu_generic_vehicles.py runs `_sweep`, the rollout and the closed-loop replay of this file on
the fully general vehicles of tests/generic_vehicles.py (`make_env` builds their configs: `generic_config`)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import generic_vehicles as GV
from tests import golden_util as G
from tests import state_blob as B
from tests.test_state_blob_cpu import ACTION_SEED, ENV_SEED, RESEAT_SEED, ROLLOUT_STEPS, STEPS, start_state

pytestmark = pytest.mark.gpu

ENV_KW = {"hexa_arm": dict(vehicle="hexa_arm"), "hexa_arm_2j": dict(vehicle="hexa_arm", n_joints=2), "hexa_arm_base": dict(vehicle="hexa_arm", ee_task="base"),
          "hexa": dict(vehicle="hexa"), "quad": dict(vehicle="quad"),
          # the fully general vehicles of tests/generic_vehicles.py: the default vehicle each of them overwrites
          "gen_quad": dict(vehicle="quad"), "gen_hexa": dict(vehicle="hexa"), "gen_arm": dict(vehicle="hexa_arm"), "gen_arm_2j": dict(vehicle="hexa_arm", n_joints=2),
          "gen_arm_base": dict(vehicle="hexa_arm", ee_task="base"), "gen_arm_yzx": dict(vehicle="hexa_arm"), "gen_arm_skew": dict(vehicle="hexa_arm")}


TASK_KW = {"v2": dict(), "v2k2": dict(num_waypoints=2), "v2k3": dict(num_waypoints=3), "v2k4": dict(num_waypoints=4), "v1_raw": dict(task="v1_raw"),
           "v1_scaled": dict(task="v1_scaled")}


def generic_config(vehicle, n, dtype="f32", kernel="auto", task="v2", seed=ENV_SEED, block_size=0):
    """The config of a "gen_..." vehicle.  GpuWaypointEnv(config=...) ignores its other keyword arguments, so this builds the config the way
    the constructor does -- default_config, seed, dtype, flags, step_kernel, block_size, the waypoint count with its trig table -- and then
    overwrites vehicle and task constants with the generic ones."""
    import math
    import rl_aerial_manipulator_amd as amd
    L = amd._lib
    kw = dict(ENV_KW[vehicle], **TASK_KW[task])
    cfg = L.default_config(kw["vehicle"], n, kw.get("task", "v2"), n_joints=kw.get("n_joints"))
    cfg.seed, cfg.dtype, cfg.flags = seed, L.F64 if dtype == "f64" else L.F32, L.FLAG_AUTO_RESET
    cfg.block_size, cfg.step_kernel = block_size, L.KERNELS[kernel]
    K = kw.get("num_waypoints", 1)
    if K != 1:
        cfg.task.num_waypoints = K
        for k in range(1, K + 1):
            t = k / K
            cfg.task.traj_sin[k - 1] = math.sin(2.0 * t * math.pi)
            cfg.task.traj_cos[k - 1] = math.cos(t * 2.0 * math.pi)
    return GV.build(cfg, vehicle)


def make_env(vehicle, n, dtype="f32", kernel="auto", task="v2", **kw):
    """kw: the constructor's other keywords; on a "gen_..." vehicle seed and block_size go into the config, the opt-in switches to the constructor."""
    import rl_aerial_manipulator_amd as amd
    if vehicle in GV.VEHICLES:
        cfg = generic_config(vehicle, n, dtype, kernel, task, **{k: kw.pop(k) for k in ("seed", "block_size") if k in kw})
        assert set(kw) <= {"randomization", "rotor_lag", "rate_control"}, kw
        return amd.GpuWaypointEnv(n, config=cfg, **kw)
    return amd.GpuWaypointEnv(n, seed=ENV_SEED, dtype=dtype, kernel=kernel, **ENV_KW[vehicle], **TASK_KW[task], **kw)


def seat(env, vehicle, n, dtype="f32", task="v2"):
    cfg, fs, is_ = start_state(vehicle, n, dtype, task)
    assert fs.shape[0] == env.n_float_fields and env.obs_dim == O.lib().orc_obs_dim(cfg)
    env.set_state(fs.copy(), is_.copy())
    return cfg, fs, is_


def gpu_state(env):
    import torch
    f, i = env.get_state()
    torch.cuda.synchronize()
    return f.cpu().numpy().astype(np.float64), i.cpu().numpy()


def gpu_step(env, a):
    """One amenv_step with every output; the per-episode rows hold a sentinel first, so that a row written for an env that did not end shows."""
    import torch
    env.terminal_obs.fill_(float("nan")); env.ep_return.fill_(float("nan")); env.ep_len.fill_(-1)
    obs, rew, done, info = env.step(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    g = dict(obs=obs.cpu().numpy().copy(), reward=rew.cpu().numpy().astype(np.float64), done=done.cpu().numpy().copy(),
             info=info.cpu().numpy().view(np.uint32).copy(), terminal_obs=env.terminal_obs.cpu().numpy().copy(),
             ep_return=env.ep_return.cpu().numpy().copy(), ep_len=env.ep_len.cpu().numpy().copy())
    g["fstate"], g["istate"] = gpu_state(env)
    return g


# (vehicle, kernel, dtype, n, substrings of kernel_name, substring that must be absent)
SWEEP = [
    ("hexa_arm", "team", "f32", 300, ("step_kernel_team<float", "helper wave per 4"), None),       # 16-env workgroups: four whole tiles and a ragged one
    ("hexa_arm", "team", "f32", 4100, ("step_kernel_team<float", "episode-end helper wave"), "per 4"),   # past 64 tiles: one integrating wave per helper
    ("hexa_arm", "team", "f64", 300, ("step_kernel_team<double",), None),
    ("hexa_arm", "staged", "f32", 300, ("step_kernel_armk<float",), None),
    ("hexa_arm", "staged", "f64", 300, ("step_kernel_armk<double",), None),
    ("hexa_arm", "helper", "f32", 300, ("step_kernel_arm2w",), None),
    ("hexa_arm", "lane", "f32", 300, ("step_kernel<float", "arm3"), None),
    ("hexa_arm", "lane", "f64", 300, ("step_kernel<double", "arm3"), None),
    ("hexa_arm_2j", "team", "f32", 300, ("step_kernel_team<float", "2-joint arm"), None),          # the caller's row widths through the pack / unpack kernels
    ("hexa_arm_base", "team", "f32", 300, ("step_kernel_team<float",), None),                      # the other task point
    ("hexa", "helper", "f32", 300, ("step_kernel_pw<float,NROT=6",), None),
    ("hexa", "lane", "f64", 300, ("step_kernel<double,NROT=6",), None),
    ("hexa", "team", "f32", 300, ("step_kernel_quad<NROT=6",), None),
    ("quad", "team", "f32", 300, ("step_kernel_quad<NROT=4",), None),
    ("quad", "helper", "f32", 300, ("step_kernel_pw<float,NROT=4",), None),
]


@pytest.mark.parametrize("vehicle,kernel,dtype,n,names,absent", SWEEP, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in SWEEP])
def test_every_branch_vs_oracle(vehicle, kernel, dtype, n, names, absent):
    _sweep(f"test_every_branch_vs_oracle[{vehicle}-{kernel}-{dtype}-{n}]", vehicle, "v2", kernel, dtype, n, names, absent)


# (vehicle, task, kernel, dtype, substrings of kernel_name).  Rigid vehicles on these tasks run the 128-thread form of step_kernel_pw: the
# main wave forms the rows, draws the next episode and writes the Monitor rows and totals itself
TASK_SWEEP = [
    ("quad", "v1_raw", "helper", "f32", ("step_kernel_pw<float,NROT=4,KW=2,v1>",)),
    ("quad", "v1_raw", "lane", "f32", ("step_kernel<float,NROT=4,KW=2,v1>",)),
    ("quad", "v1_raw", "lane", "f64", ("step_kernel<double,NROT=4,KW=2,v1>",)),
    ("quad", "v1_scaled", "helper", "f32", ("step_kernel_pw<float,NROT=4,KW=2,v1>",)),
    ("hexa", "v1_scaled", "lane", "f32", ("step_kernel<float,NROT=6,KW=2,v1>",)),
    ("quad", "v2k3", "helper", "f32", ("step_kernel_pw<float,NROT=4,KW=4,v2>",)),
    ("quad", "v2k3", "lane", "f64", ("step_kernel<double,NROT=4,KW=4,v2>",)),
    ("hexa", "v2k4", "lane", "f32", ("step_kernel<float,NROT=6,KW=4,v2>",)),
    ("hexa", "v2k2", "helper", "f32", ("step_kernel_pw<float,NROT=6,KW=4,v2>",)),
    ("hexa_arm", "v2k3", "lane", "f32", ("step_kernel<float,NROT=6,KW=4,v2+arm3>",)),
    ("hexa_arm", "v2k3", "lane", "f64", ("step_kernel<double,NROT=6,KW=4,v2+arm3>",)),
    ("hexa_arm_2j", "v2k2", "lane", "f32", ("step_kernel<float,NROT=6,KW=4,v2+arm3>", "2-joint arm", "pack / unpack")),   # the caller's row widths beside KW = 4
]


@pytest.mark.parametrize("vehicle,task,kernel,dtype,names", TASK_SWEEP, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in TASK_SWEEP])
def test_every_branch_of_the_v1_and_multi_waypoint_tasks_vs_oracle(vehicle, task, kernel, dtype, names):
    """The same sweep on the other two compile-time task forms: VAR_V1 with KW = 2 (v1_raw, v1_scaled: another state machine, the waypoint
    count per episode in the flag bits) and VAR_V2 with KW = 4 (2..4 waypoints: intermediate reaches, next-waypoint columns, hold at index K)."""
    _sweep(f"test_every_branch_of_the_v1_and_multi_waypoint_tasks_vs_oracle[{vehicle}-{task}-{kernel}-{dtype}]", vehicle, task, kernel, dtype, 300, names, None)


@pytest.mark.parametrize("vehicle,task,kernel", [("quad", "v1_raw", "team"), ("hexa", "v1_scaled", "team"), ("quad", "v2k3", "team"), ("hexa", "v2k2", "team"),
                                                 ("hexa_arm", "v2k3", "team"), ("hexa_arm", "v2k3", "staged")])
def test_families_not_built_for_these_tasks_are_refused(vehicle, task, kernel):
    """The lane-quad, lane-team and stage-wave kernels exist for the one-waypoint v2 task only: asking for them on another task is an error
    at creation, not another kernel."""
    import rl_aerial_manipulator_amd as amd
    with pytest.raises(amd.AmenvError, match=f"AMENV_KERNEL_{kernel.upper()} is built for"):
        make_env(vehicle, 300, "f32", kernel, task)


def _sweep(label, vehicle, task, kernel, dtype, n, names, absent):
    env = make_env(vehicle, n, dtype, kernel, task)
    assert all(s in env.kernel_name for s in names) and (absent is None or absent not in env.kernel_name), env.kernel_name
    cfg, _, _ = seat(env, vehicle, n, dtype, task)
    rng, rng_ld = np.random.RandomState(ACTION_SEED), np.random.RandomState(RESEAT_SEED)
    seen = {k: 0 for k in B.class_names(cfg)}
    worst = dict(state=0.0, reward=0.0, obs=0.0, ep_return=0.0, terminal_obs=0.0)
    tot = dict(episodes=0, terminated=0, truncated=0, success=0, crashed=0, oob=0, length_sum=0)
    flips = 0; ret_sum = ret_slack = 0.0
    for t in range(STEPS):
        if t:    # the last_distance a step leaves is the present distance: drawn afresh, or every slow env would sit on the progress threshold
            f, i = gpu_state(env)
            env.set_state(B.reseat_last_distance(cfg, f, rng_ld, i), i)
        pre = gpu_state(env)                                        # teacher-forced: the oracle steps the state the handle holds
        a = B.actions(cfg, pre[0], rng)
        g = gpu_step(env, a)
        o, post = B.oracle_step(cfg, pre, a)
        r = B.compare(g, o, B.margins(cfg, pre, post), dtype)
        print(f"step {t}:", {k: v for k, v in r.items() if k != "flipped"})
        flips += r["flips"]
        for k in worst:
            worst[k] = max(worst[k], r[k])
        for k, v in B.classes(cfg, pre, post, o).items():
            seen[k] += int(v.sum())
        d = o["done"] != 0
        bits = o["info"][d]
        tot["episodes"] += int(d.sum()); tot["terminated"] += int(((bits & O.INFO_TERMINATED) != 0).sum())
        tot["truncated"] += int(((bits & O.INFO_TERMINATED) == 0).sum())
        for k, b in (("success", O.INFO_SUCCESS), ("crashed", O.INFO_CRASHED), ("oob", O.INFO_OOB)):
            tot[k] += int(((bits & b) != 0).sum())
        tot["length_sum"] += int(o["ep_len"][d].sum())
        ret_sum += float(o["ep_return"][d].astype(np.float64).sum())
        # what the totals may differ by: the return gate and one unit of 2^-10 per episode; all of a flipped env's episode
        ret_slack += float((B.RET_REL * np.maximum(1.0, np.abs(o["ep_return"][d]))).sum()) + int(d.sum()) / 1024.0
        fl = r["flipped"]
        ret_slack += float(np.nan_to_num(np.abs(o["ep_return"][fl])).sum() + np.nan_to_num(np.abs(g["ep_return"][fl])).sum())
    G.report_flips(f"{label} (flag bits and rewards vs the oracle, env-steps)", flips, STEPS * n)
    print("worst errors:", worst, "branches:", seen)
    assert all(v >= 1 for v in seen.values()), seen
    st = env.stats()
    for k, v in tot.items():
        slack = flips * (cfg.task.max_episode_steps + 3) if k == "length_sum" else flips
        assert abs(st[k] - v) <= slack, (k, st[k], v, flips)
    assert st["steps"] == STEPS * n and st["nonfinite"] == 0
    assert abs(st["return_sum"] - ret_sum) <= ret_slack, (st["return_sum"], ret_sum, ret_slack)
    env.close()


def _arrived(is_):
    return (is_[O.I_FLAGS] & O.FLAGBIT_FWR) != 0


def _assert_hold_phase_reached(is_, info):
    """info [T, n] uint32 of a run from the blob: envs that had arrived hold in the first step, and a hold ends by its counter."""
    assert ((info[0] & O.INFO_SUCCESS) != 0)[_arrived(is_)].any()
    assert (((info & O.INFO_SUCCESS) != 0) & ((info & O.INFO_TERMINATED) != 0)).any()


def _assert_task_branches_reached(cfg, is_, obs, done, info, is_after):
    """Of a run from a blob of another task, obs [T, n, D], done [T, n], info [T, n] uint32, is_after the int state after it.  v1 (no hold
    phase): a final reach, and an intermediate one -- the is_final column of an env that goes on turns from 0 to 1.  v2 with several
    waypoints: the hold phase as above, and an env that went on to a later waypoint in its episode.  Both: an episode ended with a step behind it."""
    assert done[:-1].any()
    if B.is_v1(cfg):
        fl = is_[O.I_FLAGS]
        before = np.concatenate([((fl & 15) >= ((fl >> 4) & 15) - 1)[None], obs[:-1, :, 16] == 1.0])
        assert ((info & O.INFO_SUCCESS) != 0).any() and (~before & (obs[:, :, 16] == 1.0) & (done == 0)).any()
    else:
        _assert_hold_phase_reached(is_, info)
        i0, i1 = is_[O.I_FLAGS] & 15, is_after[O.I_FLAGS] & 15
        assert ((is_after[O.I_EPISODE] == is_[O.I_EPISODE]) & (i1 > i0) & (i1 < cfg.task.num_waypoints)).any()


ROLLOUT = [("hexa_arm", "v2", "team", "step_kernel_team"), ("hexa_arm", "v2", "lane", "step_kernel<float"), ("hexa", "v2", "helper", "step_kernel_pw"),
           ("quad", "v2", "team", "step_kernel_quad"), ("quad", "v1_raw", "helper", "step_kernel_pw<float,NROT=4,KW=2,v1>"),
           ("hexa", "v2k3", "lane", "step_kernel<float,NROT=6,KW=4,v2>"), ("hexa_arm", "v2k3", "lane", "step_kernel<float,NROT=6,KW=4,v2+arm3>")]


@pytest.mark.parametrize("vehicle,task,kernel,name", ROLLOUT, ids=[f"{c[0]}-{c[2]}-{c[3]}" if c[1] == "v2" else f"{c[0]}-{c[1]}-{c[2]}" for c in ROLLOUT])
def test_rollout_from_the_blob_equals_steps(vehicle, task, kernel, name):
    """amenv_rollout (its kernels carry their own episode-end path) == amenv_step launches, bit for bit, from states in the hold phase (v1:
    from states about to make their intermediate and final reaches)."""
    import torch
    n, T = 300, ROLLOUT_STEPS
    e1, e2 = make_env(vehicle, n, kernel=kernel, task=task), make_env(vehicle, n, kernel=kernel, task=task)
    assert name in e1.kernel_name
    cfg, fs, is_ = seat(e1, vehicle, n, task=task)
    seat(e2, vehicle, n, task=task)
    rng = np.random.RandomState(ACTION_SEED)
    at = torch.from_numpy(np.stack([B.actions(cfg, fs, rng) for _ in range(T)])).cuda()
    ro = e1.rollout(at)
    for t in range(T):
        obs, rew, done, info = e2.step(at[t])
        assert torch.equal(ro["obs"][t], obs) and torch.equal(ro["reward"][t], rew) and torch.equal(ro["done"][t], done) and torch.equal(ro["info_bits"][t], info), t
    f1, i1 = e1.get_state(); f2, i2 = e2.get_state()
    assert torch.equal(f1, f2) and torch.equal(i1, i2)
    s1, s2 = e1.stats(), e2.stats()
    assert s1 == s2 and s1["episodes"] == int(ro["done"].sum()) > 0 and s1["steps"] == T * n
    info = ro["info_bits"].cpu().numpy().view(np.uint32)
    if task == "v2":
        _assert_hold_phase_reached(is_, info)
    else:
        _assert_task_branches_reached(cfg, is_, ro["obs"].cpu().numpy(), ro["done"].cpu().numpy(), info, i1.cpu().numpy())
    e1.close(); e2.close()


# (vehicle, the handle's settings, the twin's settings, substring of the twin's kernel_name): the twin runs the step kernel whose arithmetic the
# closed-loop kernel of the handle carries
POLICY = [("hexa_arm", dict(kernel="team"), dict(kernel="team"), "step_kernel_team"),                       # 16 lanes per env
          ("hexa_arm", dict(kernel="lane"), dict(kernel="lane"), "step_kernel<float"),                      # one lane per env
          ("quad", dict(), dict(kernel="team"), "step_kernel_quad<NROT=4"),                                # lane-quad form, whatever kernel amenv_step runs
          ("hexa", dict(kernel="lane", block_size=64), dict(kernel="lane", block_size=64), "step_kernel<float,NROT=6"),   # a set workgroup size: one lane per env
          # the other task forms (every one of the rollout cases above: amenv_rollout_policy serves them all at 300 envs); one lane per env
          ("quad", dict(kernel="helper", task="v1_raw"), dict(kernel="lane", task="v1_raw"), "step_kernel<float,NROT=4,KW=2,v1>"),
          ("hexa", dict(kernel="lane", task="v2k3"), dict(kernel="lane", task="v2k3"), "step_kernel<float,NROT=6,KW=4,v2>"),
          ("hexa_arm", dict(kernel="lane", task="v2k3"), dict(kernel="lane", task="v2k3"), "step_kernel<float,NROT=6,KW=4,v2+arm3>")]


@pytest.mark.parametrize("vehicle,kw,twin_kw,twin_name", POLICY, ids=["hexa_arm-team", "hexa_arm-lane", "quad-lane_quad", "hexa-one_lane", "quad-v1_raw-helper",
                                                                     "hexa-v2k3-lane", "hexa_arm-v2k3-lane"])
def test_closed_loop_rollout_from_the_blob_replays_through_steps(vehicle, kw, twin_kw, twin_name):
    """amenv_rollout_policy from states in the hold phase (v1: about to make their reaches): its recorded (clipped) actions through amenv_step
    on a twin handle give the same observations, rewards, flags, terminal rows and final state bit for bit (both sides are the same fp32
    arithmetic: no env is excused)."""
    import torch
    import rl_aerial_manipulator_amd as amd
    n, T = 300, ROLLOUT_STEPS
    task = kw.get("task", "v2")
    env, twin = make_env(vehicle, n, **kw), make_env(vehicle, n, **twin_kw)
    assert twin_name in twin.kernel_name, twin.kernel_name
    cfg, fs, is_ = seat(env, vehicle, n, task=task)
    seat(twin, vehicle, n, task=task)
    od, ad, dev = env.obs_dim, env.act_dim, env.device
    torch.manual_seed(5)
    pol = amd.ActorCritic(od, ad).cuda().flatten_()
    with torch.no_grad():
        pol.log_std.data.fill_(-1.2)
        pol.action_net.weight.mul_(30.0)
    obs = torch.zeros(T + 1, n, od, device=dev); acts = torch.zeros(T, n, ad, device=dev)
    logp = torch.zeros(T, n, device=dev); vals = torch.zeros(T, n, device=dev); rew = torch.zeros(T, n, device=dev)
    dones = torch.zeros(T, n, dtype=torch.uint8, device=dev)
    info = torch.full((T, n), -1, dtype=torch.int32, device=dev)                  # 0xFFFFFFFF
    tobs = torch.full((T, n, od), float("nan"), device=dev)
    env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, obs=obs, actions=acts, logp=logp, values=vals, rewards=rew, dones=dones, info_bits=info, terminal_obs=tobs)
    torch.cuda.synchronize()
    for t in range(T):
        twin.terminal_obs.fill_(float("nan"))
        o, r, d, i = twin.step(torch.max(torch.min(acts[t], pol.action_high), pol.action_low))
        assert torch.equal(o, obs[t + 1]) and torch.equal(r, rew[t]) and torch.equal(d, dones[t]) and torch.equal(i, info[t]), t
        dn = d.bool()
        assert torch.equal(twin.terminal_obs[dn], tobs[t][dn]) and bool(torch.isnan(tobs[t][~dn]).all()), t
    f1, i1 = env.get_state(); f2, i2 = twin.get_state()
    assert torch.equal(f1, f2) and torch.equal(i1, i2)
    s1, s2 = env.stats(), twin.stats()
    assert s1 == s2 and s1["episodes"] == int(dones.sum()) > 0
    if task == "v2":
        _assert_hold_phase_reached(is_, info.cpu().numpy().view(np.uint32))
    else:
        _assert_task_branches_reached(cfg, is_, obs[1:].cpu().numpy(), dones.cpu().numpy(), info.cpu().numpy().view(np.uint32), i1.cpu().numpy())
    env.close(); twin.close()
