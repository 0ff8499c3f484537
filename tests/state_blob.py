"""Shared by tests/test_state_blob_cpu.py and tests/test_gpu_branch_sweep.py: a random state blob that reaches every branch of the v2 step
state machine on a rigid or an arm vehicle (hold phase and hold termination included), the oracle's own distance to every threshold a step
can flip, and the one routine that compares a step of the kernels with the same step of the fp64 oracle.  numpy and the oracle only: no
GPU, no torch.

Gates of `compare` (the ones tests/test_gpu_parity.py applies to the quadrotor):
  flags, done, the four int fields           equal
  float state of envs that go on             fp32: 1e-5 of max(1, |x|)   fp64: 1e-12      (every row: last_distance and ep_return too)
  state of envs that were reset              bit-equal (a pure function of seed, env id and episode)
  reward, relative to max(1, |r|)            fp32: 5e-5                  fp64: 1e-9
  observation rows, terminal rows            fp32: 1e-5 of max(1, |x|)   fp64: 1.3e-7 (one fp32 ulp: the rows are fp32)
  ep_return relative to max(1, |x|)          5e-5;  ep_len equal;  INFO_WAS_RESET exactly on the envs that ended
An env whose flag bits or reward differ is a threshold flip: allowed on fp32 only, only where the oracle's own margin to the matching
threshold is below FLIP_MARGIN, and at most flip_cap(n) per step."""
import ctypes as C

import numpy as np

from oracle import oracle as O

REL32 = 1e-5
ABS64 = 1e-12
OBS64 = 1.3e-7
REW32, REW64 = 5e-5, 1e-9
RET_REL = 5e-5
FLIP_MARGIN = 3e-5

CLASSES = ("truncated", "crashed_sinking", "crashed_rising", "oob", "first_arrival", "hold_level", "hold_tilted", "stopped", "hold_terminated",
           "arrived_outside", "progress_taken", "progress_not_taken", "last_distance_none")


def flip_cap(n):
    return max(1, n // 500)


def _cfg_for(cfg, n, flags=None):
    c = O.Config.from_buffer_copy(cfg)
    c.num_envs = n
    if flags is not None:
        c.flags = flags
    return c


def task_point(cfg, fstate):
    """[3, n]: the point the waypoint task measures from -- the tool point of an arm on its default task, the base otherwise."""
    if cfg.vehicle.n_joints and cfg.task.ee_task == O.EE_TASK_TOOL:
        e = O.OracleEnv(_cfg_for(cfg, fstate.shape[1]))
        e.fstate[:] = fstate
        return e.ee_position().T.copy()
    return fstate[0:3].copy()


def _unit(rng, n):
    v = rng.normal(size=(3, n))
    return v / np.linalg.norm(v, axis=0)


def _qmul(a, b):
    w1, x1, y1, z1 = a; w2, x2, y2, z2 = b
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def blob(cfg, n, rng):
    """(fstate [NF, n] fp64, istate [4, n] int32) for an oracle config: rigid vehicle or arm with 1..3 joints, v2 task, one waypoint.
    Generalises random_blob of tests/test_gpu_parity.py: the near-waypoint envs sit around the TASK point, a share of them has arrived
    already with counters on both sides of counter_limit, attitudes on both sides of the 0.2 rad roll / pitch bonuses, step counters on both
    sides of the time limit, last_distance far enough from the new distance that the +2 progress bonus is decided by the step's travel."""
    assert cfg.task.num_waypoints == 1 and cfg.task.variant == O.TASK_V2_SCALED20
    nj = cfg.vehicle.n_joints
    nf = O.lib().orc_n_float_fields(C.byref(cfg))
    fs = np.zeros((nf, n)); is_ = np.zeros((4, n), np.int32)
    fs[0:3] = rng.uniform(-3, 3, (3, n)); fs[2] = rng.uniform(0.05, 4, n)
    fs[3:6] = rng.normal(0, 1.0, (3, n))
    fs[10:13] = rng.normal(0, 2.0, (3, n))
    # attitudes: half uniform over the rotations; half near level with a free yaw (tilt of ~0.16 rad: both sides of the 0.2 rad bonuses)
    # (not within 0.2 rad of gimbal lock, |sin pitch| <= 0.98: there roll and yaw are atan2 of two numbers of size cos(pitch), whose fp32
    # error of ~1e-7 becomes 1e-7 / cos(pitch) in the angle and 30 / 2 pi times that in the hold reward -- measured 1.3e-4 at cos(pitch) = 1.8e-3,
    # the lane and the team kernel alike: past the 1e-5 gate on the running return by the oracle's own conditioning, not by any kernel's fault)
    q = rng.normal(size=(4, n)); q /= np.linalg.norm(q, axis=0)
    while True:
        lock = np.abs(2 * (q[0] * q[2] - q[3] * q[1])) > 0.98
        if not lock.any():
            break
        q[:, lock] = rng.normal(size=(4, int(lock.sum())))
        q /= np.linalg.norm(q, axis=0)
    psi = rng.uniform(-np.pi, np.pi, n)
    tilt = np.stack([np.ones(n), rng.normal(0, 0.08, n), rng.normal(0, 0.08, n), np.zeros(n)]); tilt /= np.linalg.norm(tilt, axis=0)
    level = _qmul(np.stack([np.cos(psi / 2), np.zeros(n), np.zeros(n), np.sin(psi / 2)]), tilt)
    fs[6:10] = np.where(rng.rand(n) < 0.5, level, q)
    j0 = O.F_WP0 + 3
    if nj:
        lim = np.array([3.1, 1.5, 1.5])[:nj, None]
        fs[j0:j0 + nj] = rng.uniform(-lim, lim, (nj, n))
        fs[j0 + nj:j0 + 2 * nj] = rng.normal(0, 1.0, (nj, n))
    near = rng.rand(n) < 0.35
    far = ~near & (rng.rand(n) < 0.05)
    fs[0:3, far] *= 4.0                                   # out of bounds
    # just above the floor (z < 0.1 ends the episode), sinking and rising by turns: both forms of the crash reward at every batch size
    # (3 % of the envs that are neither near nor far, two at the least; fast enough that one step's thrust does not turn them)
    cand = np.nonzero(~near & ~far)[0]
    low = rng.choice(cand, min(len(cand), max(2, int(0.03 * len(cand)))), replace=False)
    fs[2, low] = rng.uniform(0.05, 0.085, len(low))
    fs[5, low] = (0.3 + np.abs(fs[5, low])) * np.where(np.arange(len(low)) % 2 == 0, -1.0, 1.0)
    slow = near & (rng.rand(n) < 0.5)                     # slow enough for `stopped`
    fs[3:6, slow] *= 0.03; fs[10:13, slow] *= 0.02
    if nj:
        fs[j0 + nj:j0 + 2 * nj, slow] *= 0.02
    wp = rng.uniform(-1, 1, (3, n)); wp[2] = rng.uniform(0.5, 3, n)
    tp = task_point(cfg, fs)
    wp[:, near] = (tp + _unit(rng, n) * rng.uniform(0.0, 0.2, n))[:, near]
    fs[O.F_WP0:O.F_WP0 + 3] = wp
    fs[O.F_FINAL_YAW] = rng.uniform(-np.pi, np.pi, n)
    fs[O.F_LAST_DISTANCE] = _last_distance(np.linalg.norm(tp - wp, axis=0), rng, none_share=0.10)
    # Running return: a few units, not hundreds.  The row is gated at 1e-5 of max(1, |x|) after the step, x = return + reward, and an fp32
    # reward is a few ulp of ITS size off (measured: 1.5e-5 at r = -43, every kernel family alike).  With returns of +-100 some envs cancel to
    # |x| < 1 against a reward of 30..70 and no fp32 kernel can meet the gate there; with |return| < ~10 the sum cancels to less than 1 only
    # where the reward is small too, and above that |x| stays of the reward's size.
    fs[O.F_EP_RETURN] = rng.normal(0, 3, n)
    arrived = near & (rng.rand(n) < 0.6)
    cl, ms = cfg.task.counter_limit, cfg.task.max_episode_steps
    counter = np.where(rng.rand(n) < 0.15, rng.randint(cl - 2, cl + 4, n), rng.randint(0, cl - 2, n))
    is_[O.I_COUNTER] = np.where(arrived, counter, 0)
    is_[O.I_FLAGS] = np.where(arrived, 1 | O.FLAGBIT_FWR | O.FLAGBIT_COUNTER_ACTIVE, 0)
    is_[O.I_STEP] = np.where(rng.rand(n) < 0.05, rng.randint(ms - 3, ms + 3, n), rng.randint(0, ms - 10, n))
    is_[O.I_EPISODE] = rng.randint(1, 50, n)
    return fs, is_


def _last_distance(dist, rng, none_share):
    """last_distance for envs at distance dist: None (-1) for none_share of them; of the rest 1 in 18 within +-0.02 of dist (around the threshold
    of the +2 progress bonus), the others 0.04..0.06 away on either side: a step travels ~0.005 m, so the oracle's own margin to that
    threshold stays far above the fp32 error and the bonus still goes both ways."""
    n = len(dist)
    u = rng.rand(n)
    wide = dist + rng.uniform(0.04, 0.06, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    tight = dist + rng.normal(0, 0.01, n).clip(-0.02, 0.02)
    return np.where(u < none_share, -1.0, np.maximum(0.0, np.where(u < none_share + 0.05 * (1 - none_share) / 0.9, tight, wide)))


def reseat_last_distance(cfg, fstate, rng):
    """A copy of fstate with last_distance drawn afresh around each env's present distance, as blob() does (None stays None).  Between the
    steps of a multi-step sweep: the last_distance a step leaves IS the present distance, so that without this every slow env -- every env
    that was just reset above all -- would sit on the threshold of the progress bonus in the next step."""
    f = fstate.copy()
    dist = np.linalg.norm(task_point(cfg, f) - f[O.F_WP0:O.F_WP0 + 3], axis=0)
    f[O.F_LAST_DISTANCE] = np.where(f[O.F_LAST_DISTANCE] < 0, -1.0, _last_distance(dist, rng, none_share=0.0))
    return f


def to_f32(fstate):
    """The blob an fp32 handle holds."""
    return fstate.astype(np.float32).astype(np.float64)


def actions(cfg, fstate, rng):
    """[n, 4 + n_joints] fp32, uniform in the action box (thrust entry 0.6..1.4 with an arm); envs that turn slower than 0.08 rad/s
    hover, so that slow envs stay slow."""
    n, nj = fstate.shape[1], cfg.vehicle.n_joints
    lo = [0.6 if nj else 0.0] + [-1.0] * (3 + nj); hi = [1.4 if nj else 2.0] + [1.0] * (3 + nj)
    a = rng.uniform(lo, hi, (n, 4 + nj)).astype(np.float32)
    calm = np.linalg.norm(fstate[10:13], axis=0) < 0.08
    a[calm] = np.array([1.0] + [0.0] * (3 + nj), np.float32)
    return a


def oracle_step(cfg, pre, acts):
    """One step of the oracle from pre = (fstate, istate).  Returns (o, post): o the outputs of the oracle as cfg has it (auto-reset as
    configured) with its state after the step under "fstate" / "istate"; post = (fstate, istate, info) of a second oracle WITHOUT
    auto-reset: the post-step, pre-reset state, where the threshold margins live."""
    n = pre[0].shape[1]
    outs = []
    for flags in (cfg.flags, cfg.flags & ~O.FLAG_AUTO_RESET):
        e = O.OracleEnv(_cfg_for(cfg, n, flags))
        e.fstate[:] = pre[0]; e.istate[:] = pre[1]
        o = e.step(acts)
        o["fstate"], o["istate"] = e.fstate, e.istate
        outs.append(o)
    o, nr = outs
    return o, (nr["fstate"], nr["istate"], nr["info"])


def _rpy(q):
    w, x, y, z = q
    return np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), np.arcsin(np.clip(2 * (w * y - z * x), -1, 1))


def _geometry(cfg, pre, post):
    f0, i0 = pre
    f1 = post[0]
    d = np.linalg.norm(task_point(cfg, f1) - f1[O.F_WP0:O.F_WP0 + 3], axis=0)
    roll, pitch = _rpy(f1[6:10])
    fwr = (i0[O.I_FLAGS] & O.FLAGBIT_FWR) != 0
    return d, roll, pitch, fwr, f0[O.F_LAST_DISTANCE]


def margins(cfg, pre, post):
    """The oracle's own distance to every threshold the step from pre to post (see oracle_step) can flip, per env:
      "info":   min of |dist - 0.1|, |p_z - 0.1|, ||p| - 10|, ||v| - 0.1|, ||w| - 0.1|      (flag bits, and the reward with them)
      "reward": min of those and of the reward-only thresholds: |last_distance - dist| where the progress term counts (last_distance >= 0,
                not arrived before the step), ||roll| - 0.2| and ||pitch| - 0.2| on envs that hold after the step."""
    f1 = post[0]
    d, roll, pitch, fwr, ld = _geometry(cfg, pre, post)
    p, v, w = f1[0:3], f1[3:6], f1[10:13]
    info = np.minimum.reduce([np.abs(d - 0.1), np.abs(p[2] - 0.1), np.abs(np.linalg.norm(p, axis=0) - 10), np.abs(np.linalg.norm(v, axis=0) - 0.1),
                              np.abs(np.linalg.norm(w, axis=0) - 0.1)])
    inf = np.full(d.shape, np.inf)
    progress = np.where((ld >= 0) & ~fwr, np.abs(ld - d), inf)
    holds = fwr & (d < 0.1)
    tilt = np.where(holds, np.minimum(np.abs(np.abs(roll) - 0.2), np.abs(np.abs(pitch) - 0.2)), inf)
    return dict(info=info, reward=np.minimum.reduce([info, progress, tilt]))


def eligible(m):
    """Envs that `compare` would excuse if they flipped."""
    return m["reward"] < FLIP_MARGIN


def classes(cfg, pre, post):
    """{class: bool [n]}: the branch of the step state machine each env took in the step from pre to post (oracle_step)."""
    f1, _, info = post
    d, roll, _, fwr, ld = _geometry(cfg, pre, post)
    bit = lambda b: (info & b) != 0  # noqa: E731
    success, crashed = bit(O.INFO_SUCCESS), bit(O.INFO_CRASHED)
    counts = (ld >= 0) & ~fwr
    return dict(truncated=bit(O.INFO_TRUNCATED), crashed_sinking=crashed & (f1[5] < 0), crashed_rising=crashed & (f1[5] >= 0), oob=bit(O.INFO_OOB),
                first_arrival=success & ~fwr, hold_level=success & fwr & (np.abs(roll) < 0.2), hold_tilted=success & fwr & (np.abs(roll) >= 0.2),
                stopped=bit(O.INFO_STOPPED), hold_terminated=success & bit(O.INFO_TERMINATED), arrived_outside=fwr & ~success,
                progress_taken=counts & (ld - d > 0), progress_not_taken=counts & (ld - d <= 0), last_distance_none=ld < 0)


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _worst(x):
    return float(x.max()) if x.size else 0.0


def compare(g, o, m, dtype):
    """Assert that one step of the kernels (g) is the oracle's (o: oracle_step's first result) within the gates at the top of this file,
    m = margins(...) of that step.  Both hold obs, reward, done, info, terminal_obs, ep_return, ep_len of the step and the state after it
    under "fstate" / "istate"; rows of terminal_obs / ep_return / ep_len must have been NaN / NaN / -1 before the step (the oracle binding
    does that itself).  Returns the flip count, the flipped envs and the worst error of every gated quantity."""
    f32 = dtype == "f32"
    n = len(o["done"])
    gi, oi = np.asarray(g["info"]).view(np.uint32), np.asarray(o["info"]).view(np.uint32)
    gr, orw = np.asarray(g["reward"], np.float64), np.asarray(o["reward"], np.float64)
    gf, of = np.asarray(g["fstate"], np.float64), np.asarray(o["fstate"], np.float64)
    e_rew = np.abs(gr - orw) / np.maximum(1.0, np.abs(orw))
    flip_info = (gi & 127) != (oi & 127)
    flip_rew = ~flip_info & ~(e_rew < (REW32 if f32 else REW64))
    flips = flip_info | flip_rew
    for k in np.nonzero(flips)[0]:
        which = "info" if flip_info[k] else "reward"
        assert f32 and m[which][k] < FLIP_MARGIN, (f"env {k}: {which} differs with the oracle's margin at {m[which][k]:.3e}: info {gi[k]:#x} vs {oi[k]:#x}, "
                                                   f"reward {gr[k]!r} vs {orw[k]!r}")
    assert flips.sum() <= (flip_cap(n) if f32 else 0), f"{int(flips.sum())} threshold flips in {n} envs: {np.nonzero(flips)[0]}"
    ok = ~flips
    done = np.asarray(o["done"]) != 0
    assert np.array_equal(np.asarray(g["done"])[ok] != 0, done[ok]), "done"
    bad = ok & (np.asarray(g["istate"]) != np.asarray(o["istate"])).any(axis=0)
    assert not bad.any(), ("int fields", np.nonzero(bad)[0][:8], np.asarray(g["istate"])[:, bad][:, :8], np.asarray(o["istate"])[:, bad][:, :8])
    on, ended = ok & ~done, ok & done
    e_state = np.abs(gf - of)[:, on] if not f32 else rel_err(gf, of)[:, on]
    assert _worst(e_state) < (REL32 if f32 else ABS64), ("state of envs that go on: worst per row", e_state.max(axis=1))
    assert np.array_equal(gf[:, ended], of[:, ended]), "reset states are bit-equal"
    go, oo = np.asarray(g["obs"], np.float64), np.asarray(o["obs"], np.float64)
    obs_err = (lambda a, b: rel_err(a, b)) if f32 else (lambda a, b: np.abs(a - b))
    obs_gate = REL32 if f32 else OBS64
    e_obs = obs_err(go[ok], oo[ok])
    assert _worst(e_obs) < obs_gate, ("observation rows", _worst(e_obs))
    # ---- envs that ended, and the rows of those that did not
    was_reset = (gi & O.INFO_WAS_RESET) != 0
    assert np.array_equal(was_reset[ok], (oi[ok] & O.INFO_WAS_RESET) != 0), "INFO_WAS_RESET"
    assert np.array_equal(np.asarray(g["ep_len"])[ended], np.asarray(o["ep_len"])[ended]), "ep_len"
    e_ret = rel_err(np.asarray(g["ep_return"])[ended], np.asarray(o["ep_return"])[ended])
    assert _worst(e_ret) < RET_REL, ("ep_return", _worst(e_ret))
    e_tobs = obs_err(np.asarray(g["terminal_obs"], np.float64)[ended], np.asarray(o["terminal_obs"], np.float64)[ended])
    assert _worst(e_tobs) < obs_gate and not np.isnan(e_tobs).any(), ("terminal rows", _worst(e_tobs))
    kept = np.asarray(g["done"]) == 0
    assert np.isnan(np.asarray(g["terminal_obs"])[kept]).all() and np.isnan(np.asarray(g["ep_return"])[kept]).all() and (np.asarray(g["ep_len"])[kept] == -1).all(), \
        "rows of envs that did not end were written"
    return dict(flips=int(flips.sum()), flipped=np.nonzero(flips)[0], ended=int(ended.sum()), state=_worst(e_state), reward=_worst(e_rew[ok]), obs=_worst(e_obs),
                ep_return=_worst(e_ret), terminal_obs=_worst(e_tobs))
