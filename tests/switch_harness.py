"""What the GPU tests of the rigid vehicles' opt-in switches share: the data every one of them feeds its handles,
the bit-for-bit comparisons, one descriptor per switch, and the seven checks every switch owes -- set and cleared is invisible (open and
closed loop), one-launch rollout = T steps, the closed loop replays through amenv_step, two shards = one handle, a refused setter leaves
the handle as it was, PPO's fused rollout buffer replays.  The test files keep their cases, constants and whatever only they check."""
import dataclasses
import math
import os
import types
import typing

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
from rl_aerial_manipulator_amd.ppo import PPO, ActorCritic
from tests import delay_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- data -----------------------------------------------------------------------------------------------------------------------
def make_env(vehicle, task, nwp, n, seed=4, **kw):
    kw.setdefault("max_episode_steps", 25)
    return amd.GpuWaypointEnv(n, vehicle=vehicle, task=task, num_waypoints=nwp, seed=seed, **kw)


def actions(T, n, seed, dev, wide=False, tipped=False):
    """wide: near +-1 (and 0 / 2 on the collective), so rotors saturate at both limits and consecutive rows differ strongly.
    tipped: a third of the envs is pushed over hard, so that crashes and out-of-bounds ends join the time-limit truncations."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if wide:
        a = torch.rand(T, n, 4, generator=g)
        a = torch.where(a < 0.5, -1.0 + 0.2 * a, 0.8 + 0.4 * a)
        a[..., 0] = torch.where(a[..., 0] < 0, 1.5 + a[..., 0], a[..., 0] + 0.7)
    else:
        a = torch.rand(T, n, 4, generator=g) * torch.tensor([0.6, 0.4, 0.4, 0.4]) + torch.tensor([0.7, -0.2, -0.2, -0.2])
    if tipped:
        a[:, ::3, 0] = 0.1
        a[:, ::3, 1] = 0.9
    return a.to(dev).contiguous()


def policy(od):
    torch.manual_seed(7)
    pol = ActorCritic(od, 4).cuda().flatten_()
    with torch.no_grad():
        pol.log_std.data.fill_(-1.2)
        pol.action_net.weight.mul_(30.0)
    return pol


def fixture_policy(device):
    z = np.load(os.path.join(GOLD, "policy_2300000.npz"))
    return ActorCritic.from_sb3({k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("_")}, device=device)


def buffers(T, n, od, dev, fill=0.0):
    """fill = NaN (dones: 0xFF): a row the kernel does not write stays visible to all_written()."""
    def full(*shape):
        return torch.full(shape, fill, device=dev)
    return dict(obs=full(T + 1, n, od), actions=full(T, n, 4), logp=full(T, n), values=full(T, n), rewards=full(T, n),
                dones=torch.full((T, n), 0 if fill == 0.0 else 0xFF, dtype=torch.uint8, device=dev))


def all_written(b):
    for k, v in b.items():
        if k == "dones":
            assert bool(((v == 0) | (v == 1)).all()), "a dones entry was not written"
        else:
            assert not bool(torch.isnan(v).any()), f"a row of {k} was not written"


def step_all(env, a):
    o, r, d, i = env.step(a)
    return [x.clone() for x in (o, r, d, i, env.terminal_obs, env.ep_return, env.ep_len)], d.bool()


def oracle_cfg(env):
    return O.Config.from_buffer_copy(env.cfg)


def octo_config(n, env_id_offset=0):
    """A synthetic 8-rotor vehicle (the runtime-rotor-count kernels): rotors on a 0.3 m circle, alternating spin, pseudo-inverse allocation."""
    cfg = L.default_config("hexa", n)
    v = cfg.vehicle
    v.n_rotors, v.mass = 8, 3.0
    ang = np.arange(8) * np.pi / 4
    mix = np.stack([np.ones(8), 0.3 * np.sin(ang), -0.3 * np.cos(ang), 0.02 * (-1.0) ** np.arange(8)])
    alloc = np.linalg.pinv(mix)
    for r in range(8):
        for j in range(4):
            v.alloc[r * 4 + j] = alloc[r, j]
            v.mix[j * 8 + r] = mix[j, r]
        v.t_min[r], v.t_max[r] = 0.0, 2.0 * v.mass * v.g / 8
    cfg.env_id_offset = env_id_offset
    return cfg


def delay_history(env, z):
    """The test's own history of a handle whose delay was just turned on or that was just reset (z None: the history alone, range (0, 0))."""
    ep = env.get_state()[1][L.I_EPISODE].cpu().numpy()
    lo, hi = (0, 0) if z is None else (z.min_steps, z.max_steps)
    return delay_ref.History(env.cfg.seed, env.cfg.env_id_offset, ep, lo, hi)


def push_history(hist, env, given, info):
    reset = (info.cpu().numpy().view(np.uint32) & delay_ref.WAS_RESET) != 0
    hist.push(given.cpu().numpy(), reset, env.get_state()[1][L.I_EPISODE].cpu().numpy())
    return reset


# ---- comparisons, all bit for bit -------------------------------------------------------------------------------------------------
def same_step(ra, da, rb, db, t):
    """Two step_all() results: obs, reward, done, info everywhere; terminal_obs, ep_return, ep_len at the envs that ended (undefined elsewhere)."""
    assert len(ra) == len(rb) == 7
    for x, y in zip(ra[:4], rb[:4]):
        assert torch.equal(x, y), t
    for x, y in zip(ra[4:], rb[4:]):
        assert torch.equal(x[da], y[db]), t


def same_state(a, b, t=None):
    fa, ia = a.get_state(); fb, ib = b.get_state()
    assert torch.equal(fa, fb) and torch.equal(ia, ib), t


def same_outputs(a, b):
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


def same_tensors(xs, ys, t=None):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert torch.equal(x, y), t


# ---- the switches -----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Switch:
    kw: str                  # GpuWaypointEnv's keyword, and the attribute that holds the current value
    suffix: str              # what kernel_name carries while it is on
    setter: str
    side_state: typing.Callable   # env -> tuple of tensors: what the switch keeps beside (fstate, istate)

    def set(self, env, value):
        getattr(env, self.setter)(value)

    def same_side_state(self, a, b, t=None):
        xs = self.side_state(a)
        assert len(xs) > 0
        same_tensors(xs, self.side_state(b), t)


RANDOMIZATION = Switch("randomization", "+dr", "set_randomization", lambda e: (e.dynamics_factors(),))
ROTOR_LAG = Switch("rotor_lag", "+lag", "set_rotor_lag", lambda e: (e.rotor_state(),))
SENSOR_NOISE = Switch("sensor_noise", "+noise", "set_sensor_noise", lambda e: (e.sensor_noise_samples(),))
ACTION_DELAY = Switch("action_delay", "+delay", "set_action_delay", lambda e: tuple(e.action_delay_state()))
ACTION_HISTORY = Switch("action_history", "+history", "set_action_history", lambda e: tuple(e.action_delay_state()))


# ---- 1. set and cleared is invisible through step and rollout ---------------------------------------------------------------------
def check_same_steps_and_rollout(a, b, acts):
    """Two handles that must be indistinguishable, from where both stand: every output of every step, a rollout after it, state and totals."""
    for t in range(acts.shape[0]):
        ra, da = step_all(a, acts[t]); rb, db = step_all(b, acts[t])
        same_step(ra, da, rb, db, t)
    same_outputs(a.rollout(acts), b.rollout(acts))
    same_state(a, b)
    assert a.stats() == b.stats()


def check_set_and_cleared_step_and_rollout(sw, value, a, b, acts):
    """b has the switch set and cleared again; a never heard of it."""
    name = b.kernel_name
    sw.set(b, value)
    assert b.kernel_name == f"{name} {sw.suffix}" and getattr(b, sw.kw) is value
    sw.set(b, None)
    assert b.kernel_name == name == a.kernel_name and getattr(b, sw.kw) is None
    assert torch.equal(a.reset(), b.reset())
    check_same_steps_and_rollout(a, b, acts)


# ---- 2. ... and through the closed loop -------------------------------------------------------------------------------------------
def check_same_closed_loop(a, b, pol, T, norm=False, info_bits=True, ends=True):
    """One rollout_policy launch on each of two handles that must be indistinguishable.  norm: the normaliser inside the launch, both
    entered with the same statistics (an update's fp64 sums are atomics in no fixed order: the merged statistics agree to rounding only,
    so they are returned, a's and b's (mean, var, count), for the caller's tolerances; the rows were formed with the frozen ones)."""
    n, od, dev = a.num_envs, a.obs_dim, a.device
    ba, bb = buffers(T, n, od, dev), buffers(T, n, od, dev)
    kw_a, kw_b = {}, {}
    if info_bits:
        kw_a["info_bits"], kw_b["info_bits"] = (torch.zeros(T, n, dtype=torch.int32, device=dev) for _ in range(2))
    if norm:
        na, nb = ObsNormalizer(od), ObsNormalizer(od)
        na.update(a.observe()); nb.set(*na.get())
        kw_a["obs_normalizer"], kw_b["obs_normalizer"] = na, nb
    a.rollout_policy(pol.flat_param, T, seed=9, draw0=3, **ba, **kw_a)
    b.rollout_policy(pol.flat_param, T, seed=9, draw0=3, **bb, **kw_b)
    torch.cuda.synchronize()
    same_outputs(ba, bb)
    if info_bits:
        assert torch.equal(kw_a["info_bits"], kw_b["info_bits"])
    if ends:
        assert int(ba["dones"].sum()) > 0
    if norm:
        merged = na.get(), nb.get()
        na.close(); nb.close()
        return merged


def check_set_and_cleared_closed_loop(sw, a, b, T):
    """b was built with the switch on; a never heard of it."""
    sw.set(b, None)
    assert a.kernel_name == b.kernel_name
    a.reset(); b.reset()
    check_same_closed_loop(a, b, policy(a.obs_dim), T)
    same_state(a, b)


# ---- 3. one-launch rollout = T steps ----------------------------------------------------------------------------------------------
def check_rollout_equals_steps(a, b, acts, min_ended, side=()):
    """a.rollout(acts) against acts.shape[0] steps of its twin b; side: the switches whose side state is compared afterwards."""
    assert torch.equal(a.reset(), b.reset())
    ro = a.rollout(acts)
    for t in range(acts.shape[0]):
        o, r, d, i = b.step(acts[t])
        assert torch.equal(ro["obs"][t], o) and torch.equal(ro["reward"][t], r) and torch.equal(ro["done"][t], d) and torch.equal(ro["info_bits"][t], i), t
    assert int(ro["done"].sum()) > min_ended
    same_state(a, b)
    assert a.stats() == b.stats()
    for sw in side:
        sw.same_side_state(a, b)
    return ro


# ---- 4. the closed loop replays through amenv_step ---------------------------------------------------------------------------------
def check_closed_loop_replays(env, ref, T, norm=False, fill=0.0, side=(), prepare=None, each_step=None, totals=True):
    """One T-step rollout_policy launch on env (seed 77, draw0 5), then its recorded clipped actions through ref.step(): every row, the
    terminal rows where done, the final state, the side state of the switches in `side` and (totals) the Monitor totals are equal bit for
    bit.  norm: the normaliser inside the launch; the rows are then compared under the statistics at entry.
    prepare(env, ref) runs after both were reset (a start state of the test's own; it leaves totals that differ).
    each_step(t, given, o, r, d, i) runs after each of ref's steps, with the clipped action row and what ref.step returned.
    Returns b (the buffers), info, tobs, pol, tr (raw row -> the row the launch wrote), nrm and entry (the normaliser and its copy at
    entry, or None) and close(), which closes env, ref and the normalisers."""
    n, od, dev = env.num_envs, env.obs_dim, env.device
    pol = policy(od)
    env.reset(); ref.reset()
    if prepare is not None:
        prepare(env, ref)
    nrm = entry = None
    kw = {}
    if norm:
        nrm = ObsNormalizer(od)
        nrm.update(env.observe())
        entry = ObsNormalizer(od); entry.set(*nrm.get())
        kw = dict(obs_normalizer=nrm)
    tr = (lambda x: entry.normalize(x)) if norm else (lambda x: x)
    row0 = env.obs.clone()
    b = buffers(T, n, od, dev, fill)
    info = torch.zeros(T, n, dtype=torch.int32, device=dev); tobs = torch.full((T, n, od), float("nan"), device=dev)
    env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, info_bits=info, terminal_obs=tobs, **b, **kw)
    torch.cuda.synchronize()
    if fill != 0.0:
        all_written(b)
    assert torch.equal(b["obs"][0], tr(row0))                  # row 0: the row the handle published last
    lo, hi = pol.action_low, pol.action_high
    for t in range(T):
        given = torch.max(torch.min(b["actions"][t], hi), lo)
        o, r, d, i = ref.step(given)
        assert torch.equal(tr(o), b["obs"][t + 1]) and torch.equal(r, b["rewards"][t]) and torch.equal(d, b["dones"][t]) and torch.equal(i, info[t]), t
        dn = d.bool()
        if bool(dn.any()):
            assert torch.equal(tr(ref.terminal_obs[dn]), tobs[t][dn]), t
        if each_step is not None:
            each_step(t, given, o, r, d, i)
    same_state(env, ref)
    if totals:
        assert env.stats() == ref.stats()
    for sw in side:
        sw.same_side_state(env, ref)
    assert int(b["dones"].sum()) > 0

    def close():
        for x in (env, ref, nrm, entry):
            if x is not None:
                x.close()
    return types.SimpleNamespace(b=b, info=info, tobs=tobs, pol=pol, tr=tr, nrm=nrm, entry=entry, close=close)


# ---- 5. two shards = one handle -----------------------------------------------------------------------------------------------------
def check_two_shards(whole, h0, h1, cut, acts, side=(), every_step=False):
    """h0 holds envs [0, cut), h1 the rest (env_id_offset further by cut): rows, terminal rows and Monitor values where done, and the side
    state of the switches in `side` (after the reset and the last step; every_step: after every step) are those of the one handle."""
    def same_side(t):
        for sw in side:
            same_tensors(sw.side_state(whole), [torch.cat(p) for p in zip(sw.side_state(h0), sw.side_state(h1))], t)

    assert h0.num_envs == cut and h0.num_envs + h1.num_envs == whole.num_envs == acts.shape[1]
    ow = whole.reset().clone(); o0 = h0.reset().clone(); o1 = h1.reset().clone()
    assert torch.equal(ow, torch.cat([o0, o1]))
    same_side("reset")
    T = acts.shape[0]
    for t in range(T):
        rw, dw = step_all(whole, acts[t])
        (r0, _), (r1, _) = step_all(h0, acts[t, :cut]), step_all(h1, acts[t, cut:])
        parts = [torch.cat(p) for p in zip(r0, r1)]
        same_step(rw, dw, parts, parts[2].bool(), t)
        if every_step or t == T - 1:
            same_side(t)


# ---- 6. a refused setter -----------------------------------------------------------------------------------------------------------
def one_action(env, rows=actions):
    """rows(1, n, 3, device)[0], with zeros for an arm's joint columns."""
    a = rows(1, env.num_envs, 3, env.device)[0]
    if env.act_dim != 4:
        a = torch.cat([a, torch.zeros(env.num_envs, env.act_dim - 4, device=env.device)], dim=1).contiguous()
    return a


def next_step_alike(env, twin, action=one_action):
    a = action(env)
    same_tensors(env.step(a), twin.step(a))
    same_state(env, twin)


def check_refused(sw, make, what, match=None, action=one_action):
    """make() twice: one handle is asked for the switch -- set(what), or what(env) where `what` is the test's own way of asking -- and must
    refuse and stay as it was: state, kernel name, observe() and its next step (on the row action(env)) equal the untouched twin's."""
    env, twin = make(), make()
    env.reset(); twin.reset()
    name, (f0, i0) = env.kernel_name, env.get_state()
    if callable(what):
        what(env)
    else:
        with pytest.raises(L.AmenvError, match=match):
            sw.set(env, what)
    f1, i1 = env.get_state()
    assert torch.equal(f0, f1) and torch.equal(i0, i1)
    assert env.kernel_name == name == env.lib.amenv_kernel_name(env._h).decode() and sw.suffix not in name and getattr(env, sw.kw) is None
    assert torch.equal(env.observe(), twin.observe())
    next_step_alike(env, twin, action)
    env.close(); twin.close()


# ---- 7. PPO's fused rollout buffer replays through amenv_step -----------------------------------------------------------------------
def check_ppo_fused_rollout_replays(sw, n, T, name_ends=None, **switches):
    """Two iterations of PPO with one-launch rollouts; the first one's buffer replays through amenv_step on a lane-kernel twin."""
    env = amd.GpuWaypointEnv(n, seed=2, max_episode_steps=12, **switches)
    ref = amd.GpuWaypointEnv(n, seed=2, max_episode_steps=12, kernel="lane", **switches)
    assert env.kernel_name.endswith(name_ends or sw.suffix)
    algo = PPO(env, fused_rollout=True, n_steps=T, n_epochs=2, batch_size=8192, seed=1, bootstrap_truncated=False)
    ref.reset()
    algo.learn(T * n)
    buf = algo.buffer
    lo, hi = algo.policy.action_low, algo.policy.action_high
    for t in range(T):
        o, r, d, _ = ref.step(torch.max(torch.min(buf.actions[t], hi), lo))
        assert torch.equal(o, buf.obs[t + 1]) and torch.equal(r, buf.rewards[t]) and torch.equal(d, buf.dones[t]), t
    algo.learn(T * n)
    assert len(algo.log) == 2 and all(math.isfinite(x) for rec in algo.log for x in rec.values())
    assert int(buf.dones.sum()) > 0
    env.close(); ref.close()
