"""Every handle launches the kernels built for exactly its opt-in switches: all 16 on/off combinations of
(randomisation, rotor lag, sensor noise, actuation latency) on the quadrotor's lane kernel and the hexacopter's helper-wave kernel, through
amenv_step, amenv_rollout and -- the all-on set and each switch alone -- the closed-loop rollout.

Each switch is judged by its own device-side trace, against a twin handle with the same seed that differs in that one switch only:
  randomisation  mass range (1.5, 1.5): positions differ from the twin's;
  rotor lag      the rotor states have left their episode-start value, and positions differ from the twin's;
  sensor noise   the observation differs from the twin's in the first 13 columns of every row, while the state is the twin's bit for bit;
  latency        ActionDelay(2, 2): every d is 2, the published rows are the given ones, and the states are those of a twin given the rows
                 that were APPLIED (two hover rows first).
Within each such pair the traces of the switches the pair shares stay bit-equal wherever the differing switch cannot reach them (the rotor
states and the latency's state under the noise, the latency's state under the randomisation and the lag), and kernel_name carries exactly the
suffixes of the switches that are on.  No tolerance: every assertion is bit-equality or strict inequality.  Every handle is run once and shared."""
import functools

import pytest
import torch

import rl_aerial_manipulator_amd as amd
from tests.switch_harness import buffers, policy

pytestmark = pytest.mark.gpu

N, T = 130, 3                                          # two whole 64-env tiles and a partial one
R, L, Z, D = 1, 2, 4, 8                                # this file's numbering of the four switches
SUFFIX = {R: " +dr", L: " +lag", Z: " +noise", D: " +delay"}
FORMS = {"quad": dict(vehicle="quad", kernel="lane"), "hexa": dict(vehicle="hexa", kernel="helper")}
HOVER = torch.tensor([1.0, 0.0, 0.0, 0.0])


def _given():   # [2 T, N, 4]: T rows for the steps, T for the rollout; far from hover
    g = torch.Generator(device="cpu").manual_seed(5)
    return (torch.rand(2 * T, N, 4, generator=g) * torch.tensor([0.5, 0.6, 0.6, 0.6]) + torch.tensor([1.1, -0.3, -0.3, -0.3])).contiguous()


def _env(form, c):
    return amd.GpuWaypointEnv(N, seed=3, env_id_offset=500, **FORMS[form],
                              randomization=amd.DynamicsRandomization(mass=(1.5, 1.5)) if c & R else None,   # (mass alone: equal factors on mass and thrust cancel)
                              rotor_lag=amd.RotorLag(0.03, 0.05) if c & L else None,
                              sensor_noise=amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01) if c & Z else None,
                              action_delay=amd.ActionDelay(2, 2) if c & D else None)


def _snap(env, c):
    f, i = env.get_state()
    s = dict(f=f.cpu(), i=i.cpu())
    if c & L:
        s["w"] = env.rotor_state().cpu()
    if c & D:
        s["d"], s["recent"] = (x.cpu() for x in env.action_delay_state())
    return s


@functools.lru_cache(maxsize=None)
def _run(form, c, applied=False):
    """T steps, then a T-step rollout, of the handle with switch set c.  applied (a set without the latency): the handle is given the rows a
    d = 2 handle applies -- two hover rows, then the given rows two steps late."""
    g = _given()
    if applied:
        g = torch.cat([HOVER.expand(2, N, 4), g[:-2]]).contiguous()
    g = g.cuda()
    env = _env(form, c)
    env.reset()
    rec = dict(name=env.kernel_name, start=_snap(env, c), steps=[])
    for t in range(T):
        obs, reward, _, _ = env.step(g[t])
        rec["steps"].append(dict(obs=obs.cpu().clone(), reward=reward.cpu().clone(), **_snap(env, c)))
    out = env.rollout(g[T:])
    rec["rollout"] = dict(obs=out["obs"].cpu(), reward=out["reward"].cpu(), **_snap(env, c))
    env.close()
    return rec


def _differs_per_env(a, b):   # [fields, N] states: every env differs in at least one of its position fields
    return bool((a[:3] != b[:3]).any(dim=0).all())


def _same(a, b, keys):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("c", range(16))
@pytest.mark.parametrize("form", list(FORMS))
def test_handle_runs_its_switch_set(form, c):
    me, g = _run(form, c), _given()
    assert all((SUFFIX[s] in me["name"]) == bool(c & s) for s in SUFFIX), me["name"]
    ends = [me["steps"][-1], me["rollout"]]              # after the steps, after the rollout
    for s in (R, L, Z, D):
        if not c & s:
            continue
        tw = _run(form, c ^ s)
        tends = [tw["steps"][-1], tw["rollout"]]
        shared_d = ("d", "recent") if c & D and s != D else ()
        if s == R:
            assert all(_differs_per_env(a["f"], b["f"]) for a, b in zip(ends, tends))
            assert all(_same(a, b, shared_d) for a, b in zip(ends, tends))
        if s == L:
            assert all(bool((a["w"] != me["start"]["w"]).any(dim=1).all()) for a in ends)
            assert all(_differs_per_env(a["f"], b["f"]) for a, b in zip(ends, tends))
            assert all(_same(a, b, shared_d) for a, b in zip(ends, tends))
        if s == Z:
            rows = [(a["obs"], b["obs"]) for a, b in zip(me["steps"], tw["steps"])] + [(me["rollout"]["obs"], tw["rollout"]["obs"])]
            assert all(bool((a[..., :13] != b[..., :13]).any(dim=-1).all()) for a, b in rows)
            keep = ("f", "i", "reward") + (("w",) if c & L else ()) + shared_d
            assert all(_same(a, b, keep) for a, b in zip(me["steps"] + [me["rollout"]], tw["steps"] + [tw["rollout"]]))
        if s == D:
            for k, a in enumerate(me["steps"]):          # after step k + 1: rows k, k - 1, .. 0, hover rows behind them
                assert bool((a["d"] == 2).all())
                assert all(torch.equal(a["recent"][:, j], g[k - j] if j <= k else HOVER.expand(N, 4)) for j in range(8))
            assert bool((me["rollout"]["d"] == 2).all()) and all(torch.equal(me["rollout"]["recent"][:, j], g[2 * T - 1 - j]) for j in range(2 * T))
            ap = _run(form, c ^ D, applied=True)
            keep = ("f", "i", "reward", "obs") + (("w",) if c & L else ())
            assert all(_same(a, b, keep) for a, b in zip(me["steps"] + [me["rollout"]], ap["steps"] + [ap["rollout"]]))
            assert _differs_per_env(me["steps"][-1]["f"], tw["steps"][-1]["f"])     # (and not those of the twin given the same rows)


@pytest.mark.parametrize("c", [R | L | Z | D, R, L, Z, D])
@pytest.mark.parametrize("form", list(FORMS))
def test_closed_loop_runs_its_switch_set(form, c):
    """The closed-loop rollout picks its kernel by the same decision: a T-step launch replays bit for bit through amenv_step on a handle
    with the same switches (which the test above ties to its switch set), every switch's side state included -- with all four switches on,
    and with each one alone (where the kernel that runs is the one built with the randomisation beside it)."""
    dev = torch.device("cuda", 0)
    env, ref = _env(form, c), _env(form, c)
    env.reset(); ref.reset()
    od, start = env.obs_dim, _snap(ref, c)
    pol, b = policy(od), buffers(T, N, od, dev)
    env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, **b)
    torch.cuda.synchronize()
    assert all((SUFFIX[s] in env.kernel_name) == bool(c & s) for s in SUFFIX), env.kernel_name
    for t in range(T):
        o, r, d, _ = ref.step(torch.max(torch.min(b["actions"][t], pol.action_high), pol.action_low))
        assert torch.equal(o, b["obs"][t + 1]) and torch.equal(r, b["rewards"][t]) and torch.equal(d, b["dones"][t]), t
    a, z = _snap(env, c), _snap(ref, c)
    assert _same(a, z, tuple(a))
    if c & D:
        assert bool((a["d"] == 2).all())
    if c & L:
        assert bool((a["w"] != start["w"]).any(dim=1).all())
    env.close(); ref.close()


def test_rollout_with_history_and_lag_equals_steps():
    """amenv_rollout with the action history beside the rotor lag, on a handle of the helper form: the one combination of this file's
    kernels that nothing else launches (the history's own rollout tests run without the lag).  The rows of a T-step rollout, history
    columns included, and every side state are those of T steps on a twin handle, across an episode end that a further step follows
    (one-step time limit).  The history columns are the given rows; hover rows where the episode is younger."""
    def make():
        return amd.GpuWaypointEnv(N, seed=3, env_id_offset=500, max_episode_steps=1, **FORMS["hexa"], randomization=amd.DynamicsRandomization(mass=(1.5, 1.5)),
                                  rotor_lag=amd.RotorLag(0.03, 0.05), action_delay=amd.ActionDelay(0, 2), action_history=amd.ActionHistory(2))
    a, b = make(), make()
    a.reset(); b.reset()
    assert " +lag" in a.kernel_name and " +delay" in a.kernel_name and " +history 2" in a.kernel_name, a.kernel_name
    g = _given()[:T].cuda()
    hover = HOVER.cuda().expand(N, 4)
    ro = a.rollout(g)
    assert ro["obs"].shape == (T, N, 28)
    fresh = torch.ones(N, dtype=torch.bool, device="cuda")         # no row was given in the env's episode before this step
    for t in range(T):
        o, r, d, i = b.step(g[t])
        assert torch.equal(ro["obs"][t], o) and torch.equal(ro["reward"][t], r) and torch.equal(ro["done"][t], d) and torch.equal(ro["info_bits"][t], i), t
        new = d.bool()[:, None]                                      # (auto-reset: the row is the new episode's first)
        assert torch.equal(o[:, 20:24], torch.where(new, hover, g[t])), t
        before = g[t - 1] if t > 0 else hover                       # (t = 0: every env is fresh)
        assert torch.equal(o[:, 24:28], torch.where(new | fresh[:, None], hover, before)), t
        fresh = d.bool()
    assert bool(ro["done"][:-1].any()) and not bool(ro["done"].all())   # an episode end with a step behind it, and steps that end none
    sa, sb = _snap(a, L | D), _snap(b, L | D)
    assert _same(sa, sb, tuple(sa))
    a.close(); b.close()
