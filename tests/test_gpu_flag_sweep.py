"""Every step-kernel family under every flag word, against the fp64 oracle (`pytest -m gpu`).

`amenv_config.flags` has two bits, AMENV_FLAG_AUTO_RESET and AMENV_FLAG_NAN_GUARD, and both change the episode-end plumbing that every
family carries in its own form (`resets` in step_lane, the flag words of the helper-wave, lane-quad and lane-team kernels, the lane-team
helper's `may` predicate, the inline episode end of the rollout kernels).  tests/test_gpu_branch_sweep.py runs all of it with auto-reset
alone; here every row of its SWEEP and TASK_SWEEP (all families, fp32 and fp64, the three compile-time task forms) runs six teacher-forced
steps under
  guard_auto  NAN_GUARD | AUTO_RESET   from the POISONED blob (tests/state_blob.py `poison`: NaN, +Inf, -Inf in every guarded state row
  guard       NAN_GUARD                 and, on steps 0 and 3, in every action column; one env each, the state-poisoned ones on the
                                        workgroup / wave / tile edges 0, 15, 16, 63, 64, n - 1)
  plain       0                         from the clean blob: an env that ends is not reset and is gated like one that goes on
through `state_blob.compare` with the flag word, Monitor totals (`nonfinite` too) against the oracle's.  The contract (include/amenv.h, the
oracle is its definition): with the guard a step ends the episode with TERMINATED | NONFINITE, reward exactly -100, when (a) a state entry
is non-finite after the dynamics or (b) an entry of the action row the step applies is non-finite -- the rotor clamp would swallow (b).
(The oracle tests 13 + 2 n_joints state entries for (a), the kernels sum the 13 base entries: every joint row is poisoned here, and on
every arm kernel the base rows are non-finite after the same step, so the two agree.)
Isolation: beside a poisoned handle runs a clean twin with the guard off; every env that was never poisoned matches it bit for bit in
every output and in its state, and the rows of envs that did not end stay untouched.
Then amenv_rollout from the poisoned blob against amenv_step launches, amenv_rollout_policy from it replayed through amenv_step, and one
handle with all five opt-in switches on (the delayed action row is tested on the step that applies it).

3-joint arms run at 600 envs (78 poisoned envs are a quarter of 312), the others at 300, the lane-team kernel also at 4100.
tests/test_state_blob_cpu.py checks on the oracle alone that the poisoned blobs still reach every branch class on their clean envs, reach
every class of the guard, and that the flip cap stays a condition under every flag word.

Worst errors measured (MI355X) per flag word, over its 27 cases x 6 steps (20 fp32, 7 fp64), 0 threshold flips under every word;
NONFINITE env-steps 1560 + 585 (guard_auto), 6210 + 2310 (guard: the state poison stays), 0 (plain):
              state     reward    observation rows  ep_return  terminal rows
  guard_auto  fp32 8.7e-6   8.0e-6    4.2e-7            2.5e-6     2.3e-7        fp64 1.1e-13  1.8e-14  1.2e-7  0  1.2e-7
  guard       fp32 8.7e-6   8.0e-6    4.2e-7            3.2e-6     3.0e-7        fp64 4.5e-13  1.8e-14  1.2e-7  0  1.2e-7
  plain       fp32 8.7e-6   8.0e-6    4.2e-7            3.2e-6     3.0e-7        fp64 4.5e-13  1.8e-14  1.2e-7  0  1.2e-7
Run against the library as it was before the guard tested the action row, all 54 guarded sweep cases, all 14 rollout cases and the
switch-set case fail (the action poison is not flagged); the plain cases and the closed-loop cases (state poison only) pass."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import golden_util as G
from tests import state_blob as B
from tests.test_gpu_branch_sweep import POLICY, ROLLOUT, SWEEP, TASK_SWEEP, gpu_state, gpu_step, make_env
from tests.test_state_blob_cpu import (ACTION_POISON_STEPS, ACTION_SEED, ENV_SEED, FLAG_STATES, FLAG_WORDS, RESEAT_SEED, ROLLOUT_STEPS, STEPS, flag_actions, flag_n,
                                       poisoned_start, start_state)

pytestmark = pytest.mark.gpu

WORDS = list(FLAG_WORDS)


def _bits(word):
    f = FLAG_WORDS[word]
    return f, (f & O.FLAG_NAN_GUARD) != 0, (f & O.FLAG_AUTO_RESET) != 0


def _finite_or_zero(x):
    x = np.asarray(x, np.float64)
    return np.where(np.isfinite(x), x, 0.0)


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("vehicle,kernel,dtype,n,names,absent", SWEEP, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in SWEEP])
def test_every_family_under_every_flag_word_vs_oracle(vehicle, kernel, dtype, n, names, absent, word):
    _flag_sweep(f"test_every_family_under_every_flag_word_vs_oracle[{vehicle}-{kernel}-{dtype}-{n}-{word}]", vehicle, "v2", kernel, dtype, n, names, absent, word)


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("vehicle,task,kernel,dtype,names", TASK_SWEEP, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in TASK_SWEEP])
def test_the_v1_and_multi_waypoint_task_forms_under_every_flag_word_vs_oracle(vehicle, task, kernel, dtype, names, word):
    """`task_step_v1` has a guard return of its own, and the KW = 4 kernels their own episode-end paths."""
    _flag_sweep(f"test_the_v1_and_multi_waypoint_task_forms_under_every_flag_word_vs_oracle[{vehicle}-{task}-{kernel}-{dtype}-{word}]", vehicle, task, kernel, dtype, 300,
                names, None, word)


def _flag_sweep(label, vehicle, task, kernel, dtype, n, names, absent, word):
    flags, guard, auto = _bits(word)
    n = flag_n(vehicle, n)
    assert (vehicle, n, dtype, task) in FLAG_STATES                     # the oracle-alone test has vouched for these states
    env = make_env(vehicle, n, dtype, kernel, task, auto_reset=auto, nan_guard=guard)
    assert all(s in env.kernel_name for s in names) and (absent is None or absent not in env.kernel_name), env.kernel_name
    if guard:
        cfg, fs, is_, masks = poisoned_start(vehicle, n, dtype, task)
    else:
        (cfg, fs, is_), masks = start_state(vehicle, n, dtype, task), None
    cfg, tcfg = B._cfg_for(cfg, n, flags), B._cfg_for(cfg, n, flags & ~O.FLAG_NAN_GUARD)
    assert fs.shape[0] == env.n_float_fields and env.obs_dim == O.lib().orc_obs_dim(cfg)
    env.set_state(fs.copy(), is_.copy())
    twin = None
    if guard:      # the clean twin: guard off, the unpoisoned blob, the same draws
        twin = make_env(vehicle, n, dtype, kernel, task, auto_reset=auto, nan_guard=False)
        assert twin.kernel_name == env.kernel_name
        twin.set_state(start_state(vehicle, n, dtype, task)[1].copy(), is_.copy())
    clean = masks["clean"] if guard else np.ones(n, bool)
    rngs = [(np.random.RandomState(ACTION_SEED), np.random.RandomState(RESEAT_SEED)) for _ in range(2)]
    class_names = [k for k in B.class_names(cfg) if auto or not k.startswith("reset_drew")]      # (without auto-reset no reset draws anything)
    seen, seen_nf = {k: 0 for k in class_names}, {k: 0 for k in B.nonfinite_class_names(cfg)}
    worst = dict(state=0.0, reward=0.0, obs=0.0, ep_return=0.0, terminal_obs=0.0)
    tot = dict(episodes=0, terminated=0, truncated=0, success=0, crashed=0, oob=0, nonfinite=0, length_sum=0)
    flips = 0; ret_sum = ret_slack = 0.0
    for t in range(STEPS):
        if t:    # the last_distance a step leaves is the present distance: drawn afresh (tests/test_gpu_branch_sweep.py)
            for e, c, (_, rl) in ((env, cfg, rngs[0]), (twin, tcfg, rngs[1])):
                if e is not None:
                    f, i = gpu_state(e)
                    with np.errstate(invalid="ignore"):
                        e.set_state(B.reseat_last_distance(c, f, rl, i), i)
        pre = gpu_state(env)                                        # teacher-forced: the oracle steps the state the handle holds
        a = flag_actions(cfg, pre, rngs[0][0], t, masks)
        g = gpu_step(env, a)
        with np.errstate(invalid="ignore"):
            o, post = B.oracle_step(cfg, pre, a)
            r = B.compare(g, o, B.margins(cfg, pre, post), dtype, flags)
            cl = B.classes(cfg, pre, post, o)
        print(f"step {t}:", {k: v for k, v in r.items() if k != "flipped"})
        flips += r["flips"]
        for k in worst:
            worst[k] = max(worst[k], r[k])
        for k in class_names:
            seen[k] += int((cl[k] & clean).sum())
        nf = (g["info"] & O.INFO_NONFINITE) != 0
        assert not nf[clean].any(), ("a clean env was flagged", t, np.nonzero(nf & clean)[0])
        if guard:
            # ---- what the poison must do
            if t == 0 or not auto:
                assert nf[masks["state"]].all(), (t, "state poison not flagged", np.nonzero(masks["state"] & ~nf)[0])
            if t in ACTION_POISON_STEPS:
                assert nf[masks["action"]].all(), (t, "action poison not flagged", np.nonzero(masks["action"] & ~nf)[0])
            assert np.array_equal((g["info"][nf] & O.INFO_WAS_RESET) != 0, np.full(int(nf.sum()), auto)), (t, "a NONFINITE env is reset exactly with auto-reset")
            # ---- isolation: the envs that were never poisoned are, bit for bit, those of the clean twin
            tpre = gpu_state(twin)
            ta = flag_actions(tcfg, tpre, rngs[1][0], t, None)
            assert np.array_equal(a[clean], ta[clean])
            tg = gpu_step(twin, ta)
            for k in ("obs", "reward", "done", "info", "terminal_obs", "ep_return", "ep_len"):
                assert np.array_equal(g[k][clean], tg[k][clean], equal_nan=True), (t, k, "a clean env differs from the clean twin")
            assert np.array_equal(g["fstate"][:, clean], tg["fstate"][:, clean]) and np.array_equal(g["istate"][:, clean], tg["istate"][:, clean]), (t, "state")
            _, tpost = B.oracle_step(tcfg, tpre, ta)
            for k, v in B.nonfinite_classes(cfg, pre, a, g["info"], B._geometry(tcfg, tpre, tpost)[0]).items():
                seen_nf[k] += int(v.sum())
        d = o["done"] != 0
        bits = o["info"][d]
        tot["episodes"] += int(d.sum()); tot["terminated"] += int(((bits & O.INFO_TERMINATED) != 0).sum())
        tot["truncated"] += int(((bits & O.INFO_TERMINATED) == 0).sum())
        for k, b in (("success", O.INFO_SUCCESS), ("crashed", O.INFO_CRASHED), ("oob", O.INFO_OOB), ("nonfinite", O.INFO_NONFINITE)):
            tot[k] += int(((bits & b) != 0).sum())
        tot["length_sum"] += int(o["ep_len"][d].sum())
        ret = _finite_or_zero(o["ep_return"][d])                    # (a return that is not finite adds nothing to the total)
        ret_sum += float(ret.sum())
        ret_slack += float((B.RET_REL * np.maximum(1.0, np.abs(ret))).sum()) + int(d.sum()) / 1024.0
        fl = r["flipped"]
        ret_slack += float(np.abs(_finite_or_zero(o["ep_return"][fl])).sum() + np.abs(_finite_or_zero(g["ep_return"][fl])).sum())
    G.report_flips(f"{label} (flag bits and rewards vs the oracle, env-steps)", flips, STEPS * n)
    print(f"FLAGSWEEP {word} flips {flips} worst {worst} nonfinite {tot['nonfinite']} branches {seen} guard classes {seen_nf}")
    assert all(v >= 1 for v in seen.values()), seen
    assert not guard or all(v >= 1 for v in seen_nf.values()), seen_nf
    st = env.stats()
    for k, v in tot.items():
        slack = flips * (cfg.task.max_episode_steps + 3) if k == "length_sum" else (0 if k == "nonfinite" else flips)
        assert abs(st[k] - v) <= slack, (k, st[k], v, flips)
    assert st["steps"] == STEPS * n and (st["nonfinite"] > 0) == guard
    assert abs(st["return_sum"] - ret_sum) <= ret_slack, (st["return_sum"], ret_sum, ret_slack)
    env.close()
    if twin is not None:
        assert twin.stats()["nonfinite"] == 0
        twin.close()


def _eq(a, b):
    """Bit for bit, NaN positions equal."""
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("word", ["guard_auto", "guard"])
@pytest.mark.parametrize("vehicle,task,kernel,name", ROLLOUT, ids=[f"{c[0]}-{c[2]}-{c[3]}" if c[1] == "v2" else f"{c[0]}-{c[1]}-{c[2]}" for c in ROLLOUT])
def test_rollout_from_the_poisoned_blob_equals_steps(vehicle, task, kernel, name, word):
    """amenv_rollout (its kernels carry their own episode-end path) == amenv_step launches with the guard on, bit for bit, NaN positions
    equal.  Unspecified and skipped: the row and the float state of an env that is NONFINITE and not reset.  With auto-reset the action
    poison comes on steps 0 and 2; without it on the last step (the float state such a step leaves is unspecified, and every later step
    would start from it)."""
    import torch
    flags, guard, auto = _bits(word)
    n, T = flag_n(vehicle, 300), ROLLOUT_STEPS
    e1, e2 = (make_env(vehicle, n, kernel=kernel, task=task, auto_reset=auto, nan_guard=True) for _ in range(2))
    assert name in e1.kernel_name
    cfg, fs, is_, masks = poisoned_start(vehicle, n, "f32", task)
    e1.set_state(fs.copy(), is_.copy()); e2.set_state(fs.copy(), is_.copy())
    rng = np.random.RandomState(ACTION_SEED)
    poison_at = (0, 2) if auto else (T - 1,)
    acts = [B.actions(cfg, fs, rng) for _ in range(T)]
    at = torch.from_numpy(np.stack([B.poison_actions(a, masks) if t in poison_at else a for t, a in enumerate(acts)])).cuda()
    ro = e1.rollout(at)
    stale = np.zeros(n, bool)
    for t in range(T):
        obs, rew, done, info = e2.step(at[t])
        assert torch.equal(ro["done"][t], done) and torch.equal(ro["info_bits"][t], info) and _eq(ro["reward"][t], rew), t
        bits = info.cpu().numpy().view(np.uint32)
        nf = (bits & O.INFO_NONFINITE) != 0
        stale = nf & ((bits & O.INFO_WAS_RESET) == 0)
        assert _eq(ro["obs"][t][torch.from_numpy(~stale).cuda()], obs[torch.from_numpy(~stale).cuda()]), t
        assert (t != 0 and auto) or nf[masks["state"]].all(), t
        assert nf[masks["action"]].all() if t in poison_at else True, t
        assert not nf[masks["clean"]].any() and (rew.cpu().numpy()[nf] == -100.0).all() and np.array_equal((bits[nf] & O.INFO_WAS_RESET) != 0, np.full(int(nf.sum()), auto)), t
    f1, i1 = e1.get_state(); f2, i2 = e2.get_state()
    keep = torch.from_numpy(~stale).cuda()
    assert _eq(f1[:, keep], f2[:, keep]) and torch.equal(i1, i2)
    assert auto == bool(torch.isfinite(f1).all())
    s1, s2 = e1.stats(), e2.stats()
    assert s1 == s2 and s1["episodes"] == int(ro["done"].sum()) > 0 and s1["steps"] == T * n and s1["nonfinite"] >= int(masks["state"].sum() + masks["action"].sum())
    e1.close(); e2.close()


@pytest.mark.parametrize("vehicle,kw,twin_kw,twin_name", POLICY, ids=["hexa_arm-team", "hexa_arm-lane", "quad-lane_quad", "hexa-one_lane", "quad-v1_raw-helper",
                                                                     "hexa-v2k3-lane", "hexa_arm-v2k3-lane"])
def test_closed_loop_rollout_from_the_poisoned_blob_replays_through_steps(vehicle, kw, twin_kw, twin_name):
    """amenv_rollout_policy from the state-poisoned blob under NAN_GUARD | AUTO_RESET: its recorded (clipped) actions through amenv_step on
    a twin handle give the same observations, rewards, flags and final state bit for bit, the same terminal rows except those of the
    NONFINITE envs (unspecified), and the same Monitor totals with nonfinite > 0."""
    import torch
    import rl_aerial_manipulator_amd as amd
    n, T = flag_n(vehicle, 300), ROLLOUT_STEPS
    task = kw.get("task", "v2")
    env, twin = make_env(vehicle, n, nan_guard=True, **kw), make_env(vehicle, n, nan_guard=True, **twin_kw)
    assert twin_name in twin.kernel_name, twin.kernel_name
    cfg, fs, is_, masks = poisoned_start(vehicle, n, "f32", task)
    env.set_state(fs.copy(), is_.copy()); twin.set_state(fs.copy(), is_.copy())
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
        nf = (i & int(O.INFO_NONFINITE)) != 0
        dn = d.bool() & ~nf
        assert torch.equal(twin.terminal_obs[dn], tobs[t][dn]) and bool(torch.isnan(tobs[t][~d.bool()]).all()), t
        poisoned = torch.from_numpy(masks["state"]).to(dev)
        assert (bool(nf[poisoned].all()) if t == 0 else not bool(nf[poisoned].any())) and not bool(nf[~poisoned].any()), t
        assert bool((r[nf] == -100.0).all()) and bool(((i[nf] & int(O.INFO_WAS_RESET)) != 0).all())
    f1, i1 = env.get_state(); f2, i2 = twin.get_state()
    assert torch.equal(f1, f2) and torch.equal(i1, i2) and bool(torch.isfinite(f1).all())
    s1, s2 = env.stats(), twin.stats()
    assert s1 == s2 and s1["episodes"] == int(dones.sum()) > 0 and s1["nonfinite"] == int(masks["state"].sum())
    env.close(); twin.close()


def test_guard_on_a_handle_with_every_opt_in_switch_on():
    """Quadrotor, one lane per env, dynamics randomisation, rotor lag, sensor noise, action delay (2 steps) and action history on: with
    the guard, clean envs are bit-equal to the same handle with the guard off, state-poisoned envs are flagged and reset, and a non-finite
    row that goes into the delay history is flagged on the step that applies it, not on the step that receives it."""
    import torch
    import rl_aerial_manipulator_amd as amd
    n, T, D = 300, 5, 2
    cfg, fs, is_, masks = poisoned_start("quad", n, "f32", "v2")
    clean_fs = start_state("quad", n, "f32", "v2")[1]

    def handle(guard, state):
        env = amd.GpuWaypointEnv(n, seed=ENV_SEED, kernel="lane", nan_guard=guard)
        env.set_randomization(amd.DynamicsRandomization(mass=(0.8, 1.25), thrust=(0.9, 1.1))); env.set_rotor_lag(amd.RotorLag(0.03, 0.05))
        env.set_sensor_noise(amd.SensorNoise(position=0.02)); env.set_action_delay(amd.ActionDelay(D, D)); env.set_action_history(amd.ActionHistory(2))
        assert all(s in env.kernel_name for s in ("+dr", "+lag", "+noise", "+delay", "+history 2")), env.kernel_name
        env.set_state(state.copy(), is_.copy())
        return env

    on, off = handle(True, fs), handle(False, clean_fs)
    late = np.nonzero(masks["clean"] & (is_[O.I_STEP] < 100))[0][:9]              # envs that are given a non-finite row on step 1
    clean = ~masks["state"]; clean[late] = False
    rng = np.random.RandomState(ACTION_SEED)
    bits, dones = [], []
    for t in range(T):
        a = B.actions(cfg, clean_fs, rng)
        bad = a.copy()
        if t == 1:
            for j, k in enumerate(late):
                bad[k, j % 4] = B.POISON_VALUES[j % 3]
        o1, r1, d1, i1 = (x.cpu().numpy().copy() for x in on.step(torch.from_numpy(bad).cuda()))
        o0, r0, d0, i0 = (x.cpu().numpy().copy() for x in off.step(torch.from_numpy(a).cuda()))
        assert np.array_equal(o1[clean], o0[clean]) and np.array_equal(r1[clean], r0[clean]) and np.array_equal(d1[clean], d0[clean]) and np.array_equal(i1[clean], i0[clean]), t
        i1 = i1.view(np.uint32)
        nf = (i1 & O.INFO_NONFINITE) != 0
        assert not nf[clean].any() and nf[masks["state"]].all() == (t == 0) and (t == 0 or not nf[masks["state"]].any()), t
        assert ((i1[nf] & O.INFO_WAS_RESET) != 0).all() and (r1[nf] == -100.0).all()
        if t < 1 + D:      # the step that receives the row, and the steps before it is applied: as the handle that was given a finite one
            assert not nf[late].any() and np.array_equal(r1[late], r0[late]) and np.array_equal(i1[late], i0[late].view(np.uint32)), t
        bits.append(nf); dones.append(d0 != 0)
    waited = ~(dones[1][late] | dones[2][late])                                    # (a reset between the two steps wipes the history)
    assert waited.sum() >= 3 and bits[1 + D][late][waited].all() and not bits[1 + D][late][~waited].any() and not bits[T - 1][late].any()
    (f1, s1), (f0, s0) = gpu_state(on), gpu_state(off)
    assert np.array_equal(f1[:, clean], f0[:, clean]) and np.array_equal(s1[:, clean], s0[:, clean]) and np.isfinite(f1).all()
    assert on.stats()["nonfinite"] == int(masks["state"].sum() + waited.sum()) and off.stats()["nonfinite"] == 0
    on.close(); off.close()
