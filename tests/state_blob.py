"""Shared by tests/test_state_blob_cpu.py and tests/test_gpu_branch_sweep.py: a random state blob that reaches every branch of the step
state machine of the config's task -- v2 with 1..4 waypoints on a rigid or an arm vehicle (hold phase and hold termination included,
intermediate reaches with several waypoints), or v1 (raw or scaled rows) on a rigid vehicle --, the oracle's own distance to every threshold
a step can flip, and the one routine that compares a step of the kernels with the same step of the fp64 oracle.  numpy and the oracle only:
no GPU, no torch.

Gates of `compare` (the ones tests/test_gpu_parity.py applies to the quadrotor):
  flags, done, the four int fields           equal
  float state of envs that go on             fp32: 1e-5 of max(1, |x|)   fp64: 1e-12      (every row: last_distance and ep_return too)
  state of envs that were reset              bit-equal (a pure function of seed, env id and episode)
  reward, relative to max(1, |r|)            fp32: 5e-5                  fp64: 1e-9
  observation rows, terminal rows            fp32: 1e-5 of max(1, |x|)   fp64: 1.3e-7 (one fp32 ulp: the rows are fp32)
  ep_return relative to max(1, |x|)          5e-5;  ep_len equal;  INFO_WAS_RESET exactly on the envs that ended
An env whose flag bits or reward differ is a threshold flip: allowed on fp32 only, only where the oracle's own margin to the matching
threshold is below FLIP_MARGIN, and at most flip_cap(n) per step.

The flag word (tests/test_gpu_flag_sweep.py).  `compare` takes the handle's flags: without AMENV_FLAG_AUTO_RESET an env that ended is not
reset and is gated like one that goes on.  With AMENV_FLAG_NAN_GUARD, `poison` puts NaN, +Inf and -Inf into every guarded state row and every
action column, one env each; an env the oracle or the kernels flag NONFINITE is never an excusable flip: flag bits, done, the int fields,
ep_len equal, reward exactly -100, ep_return within RET_REL where the oracle's is finite, reset state bit-equal and post-reset row within
the row gate when it was reset.  Its terminal row, its row and its float state when it was not reset are unspecified (include/amenv.h) and
skipped."""
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
# v2 with 2..4 waypoints: those, and the branches only an intermediate waypoint has
CLASSES_MULTI = CLASSES + ("intermediate_reach", "intermediate_reach_then_crash_or_oob", "final_first_arrival", "next_waypoint_columns_nonzero",
                           "next_waypoint_columns_zero")
# v1 (both variants): another state machine -- no hold phase, a per-episode waypoint count, +-10 approach shaping, a final reach that returns
# before the step counter moves
CLASSES_V1 = ("truncated", "crashed_sinking", "crashed_rising", "oob", "intermediate_reach", "final_reach_stopped", "final_reach_moving",
              "final_reach_at_time_limit", "shaping_plus", "shaping_minus", "shaping_off", "progress_taken", "progress_not_taken", "last_distance_none",
              "is_final_0", "is_final_1", "reset_drew_k1", "reset_drew_k2")


def is_v1(cfg):
    return cfg.task.variant in (O.TASK_V1_SCALED17, O.TASK_V1_RAW17)


def class_names(cfg):
    """The classes `classes` reports for cfg's task."""
    if is_v1(cfg):
        return CLASSES_V1
    return CLASSES if cfg.task.num_waypoints == 1 else CLASSES_MULTI


# the guard's own classes (tests/test_state_blob_cpu.py reaches each on the oracle alone); v1 has no hold phase
CLASSES_NONFINITE = ("nonfinite_state", "nonfinite_action", "nonfinite_at_time_limit", "nonfinite_while_holding", "nonfinite_that_would_have_reached")
POISON_VALUES = (np.nan, np.inf, -np.inf)
POISON_SHARE = 0.25          # poisoned envs are at most this share of the batch: the branch classes live on the others
EDGE_ENVS = (0, 15, 16, 63, 64, -1)   # workgroup, wave and tile edges of the 16-, 64- and 256-lane forms, and the ragged tail


def nonfinite_class_names(cfg):
    return tuple(k for k in CLASSES_NONFINITE if not (is_v1(cfg) and k == "nonfinite_while_holding"))


def flip_cap(n):
    return max(1, n // 500)


def guarded_rows(cfg):
    """The float-state rows AMENV_FLAG_NAN_GUARD tests: the 13 base entries, joint angles and joint rates."""
    j0 = O.F_WP0 + 3 * cfg.task.num_waypoints
    return list(range(13)) + list(range(j0, j0 + 2 * cfg.vehicle.n_joints))


def poison(cfg, fstate, acts, rng, must=(), avoid=None):
    """(fstate, acts, masks): copies with NaN, +Inf and -Inf in every guarded state row and every action column, one env per (row, value)
    and per (column, value).  The state-poisoned envs include EDGE_ENVS and `must` (envs the caller wants flagged: at the time limit,
    holding, about to reach); the others are drawn from the envs outside `avoid` (bool [n]: envs a branch class needs).  masks: "state" /
    "action" bool [n], "clean" = neither; "state_env" / "action_env" the envs in (row, value) / (column, value) order."""
    n = fstate.shape[1]
    rows, cols = guarded_rows(cfg), range(acts.shape[1])
    ns, na = len(rows) * len(POISON_VALUES), len(cols) * len(POISON_VALUES)
    assert ns + na <= POISON_SHARE * n, f"{ns + na} poisoned envs of {n}: more than {POISON_SHARE:.0%} (raise n)"
    fixed = list(dict.fromkeys([e % n for e in EDGE_ENVS] + [int(e) for e in must]))
    free = np.ones(n, bool) if avoid is None else ~np.asarray(avoid)
    free[fixed] = False
    drawn = rng.choice(np.nonzero(free)[0], ns + na - len(fixed), replace=False)
    state_env = np.array(fixed + list(drawn[:ns - len(fixed)])); action_env = drawn[ns - len(fixed):]
    state_env = state_env[rng.permutation(ns)]                # which (row, value) an edge env gets is drawn too
    f = fstate.copy()
    k = 0
    for r in rows:
        for v in POISON_VALUES:
            f[r, state_env[k]] = v; k += 1
    ms, ma = np.zeros(n, bool), np.zeros(n, bool)
    ms[state_env] = True; ma[action_env] = True
    masks = dict(state=ms, action=ma, clean=~(ms | ma), state_env=state_env, action_env=action_env)
    return f, poison_actions(acts, masks), masks


def poison_actions(acts, masks):
    """A copy of acts with the action poison of `poison` put in: the same (column, value) on the same envs, on another step's rows."""
    a = acts.copy()
    k = 0
    for c in range(acts.shape[1]):
        for v in POISON_VALUES:
            a[masks["action_env"][k], c] = v; k += 1
    return a


def nonfinite_classes(cfg, pre, acts, info, clean_distance):
    """{class: bool [n]} of the guard's own branches in one step: info the step's flag bits, acts the rows it applied, clean_distance the
    distance the same step of the unpoisoned twin measured (NaN where there is none)."""
    nf = (np.asarray(info).view(np.uint32) & O.INFO_NONFINITE) != 0
    bad_a = ~np.isfinite(acts).all(axis=1)
    c = dict(nonfinite_state=nf & ~bad_a, nonfinite_action=nf & bad_a, nonfinite_at_time_limit=nf & ((info & O.INFO_TRUNCATED) != 0),
             nonfinite_while_holding=nf & ((pre[1][O.I_FLAGS] & O.FLAGBIT_FWR) != 0), nonfinite_that_would_have_reached=nf & (clean_distance < 0.1))
    return {k: c[k] for k in nonfinite_class_names(cfg)}


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


def current_waypoint(cfg, fstate, istate):
    """([3, n] the waypoint each env flies to, its slot [n], the waypoint count [n]): slot = min(index, K - 1), K from flag bits 4-7 on the
    v1 tasks (drawn per episode) and from the config on v2."""
    n = fstate.shape[1]
    fl = istate[O.I_FLAGS]
    K = ((fl >> 4) & 15) if is_v1(cfg) else np.full(n, cfg.task.num_waypoints)
    slot = np.minimum(fl & 15, K - 1)
    cols = np.arange(n)
    return np.stack([fstate[O.F_WP0 + 3 * slot + c, cols] for c in range(3)]), slot, K


def blob(cfg, n, rng):
    """(fstate [NF, n] fp64, istate [4, n] int32) for an oracle config: rigid vehicle or arm with 1..3 joints on the v2 task with 1..4
    waypoints, or a rigid vehicle on a v1 task.
    Generalises random_blob of tests/test_gpu_parity.py: the near-waypoint envs sit around the TASK point, a share of them has arrived
    already with counters on both sides of counter_limit, attitudes on both sides of the 0.2 rad roll / pitch bonuses, step counters on both
    sides of the time limit, last_distance far enough from the new distance that the +2 progress bonus is decided by the step's travel.
    The draws common to all tasks come first and in one order, the task's own after them: with one waypoint on v2 the states are those of
    the first version of this file bit for bit (tests/test_state_blob_cpu.py pins their checksums).
      v2, K > 1: every slot filled, the index spread over 0..K-1 (arrived envs: K with both phase bits), near envs around the task point of
        their CURRENT waypoint, a few of those that will reach an intermediate waypoint moved below z = 0.1 (waypoint moved along).
      v1: a waypoint count of 1 or 2 per env in flag bits 4-7 (one: second slot zero, as the reset leaves it), index below it, no phase
        bits and no counter; near envs up to 0.6 m from the current waypoint (both sides of 0.1 and of 0.5), the fast ones flying toward it,
        away from it or as drawn; final reaches with the step counter at and past the time limit."""
    v1 = is_v1(cfg)
    K = cfg.task.num_waypoints
    nj = cfg.vehicle.n_joints
    assert (v1 and K == 2 and nj == 0) or (cfg.task.variant == O.TASK_V2_SCALED20 and 1 <= K <= O.MAX_WAYPOINTS), (cfg.task.variant, K, nj)
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
    j0 = O.F_WP0 + 3 * K
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
    wps = np.zeros((K, 3, n))
    wps[0] = rng.uniform(-1, 1, (3, n)); wps[0, 2] = rng.uniform(0.5, 3, n)
    tp = task_point(cfg, fs)
    off_dir = _unit(rng, n); off_len = rng.uniform(0.0, 0.2, n)      # near envs: from the task point to the current waypoint
    fs[O.F_FINAL_YAW] = rng.uniform(-np.pi, np.pi, n)
    ld = _last_distance_draws(rng, n)
    # Running return: a few units, not hundreds.  The row is gated at 1e-5 of max(1, |x|) after the step, x = return + reward, and an fp32
    # reward is a few ulp of ITS size off (measured: 1.5e-5 at r = -43, every kernel family alike).  With returns of +-100 some envs cancel to
    # |x| < 1 against a reward of 30..70 and no fp32 kernel can meet the gate there; with |return| < ~10 the sum cancels to less than 1 only
    # where the reward is small too, and above that |x| stays of the reward's size.
    fs[O.F_EP_RETURN] = rng.normal(0, 3, n)
    arrived = near & (rng.rand(n) < 0.6)
    cl, ms = cfg.task.counter_limit, cfg.task.max_episode_steps
    counter = np.where(rng.rand(n) < 0.15, rng.randint(cl - 2, cl + 4, n), rng.randint(0, cl - 2, n))
    is_[O.I_STEP] = np.where(rng.rand(n) < 0.05, rng.randint(ms - 3, ms + 3, n), rng.randint(0, ms - 10, n))
    is_[O.I_EPISODE] = rng.randint(1, 50, n)
    # ---- the task's own part
    cols = np.arange(n)
    for k in range(1, K):
        wps[k] = rng.uniform(-1, 1, (3, n)); wps[k, 2] = rng.uniform(0.5, 3, n)
    if v1:
        arrived[:] = False                                # no hold phase
        kep = rng.randint(1, 3, n)
        slot = rng.randint(0, 2, n) % kep
        wps[1][:, kep == 1] = 0.0
        # Distance of the near envs: up to 0.6 m, and not below 2e-3 (slow envs) / 2e-2 (the others).  The shaping compares
        # vtw = v . d / |d| with 0.1, d = waypoint - position: an fp32 position of 1..4 m carries ~1.2e-7, so the direction d / |d| carries
        # 1.2e-7 / |d| and vtw that times the speed.  Measured on the post-step states of this blob (numpy: state within one fp32 rounding
        # of the oracle's, vtw formed in fp32 as the kernels form it, against the oracle's fp64 value): 2.2e-5 at |d| = 2.3e-2 and
        # |v| = 2.8, i.e. 1.8e-7 |v| / |d|, just below FLIP_MARGIN -- at 2e-3 it would be 2.5e-4, and a flip there would be the oracle's own
        # conditioning and no kernel's fault; the slow envs (|v| < 0.07) stay below 1.5e-6 down to 4e-3.  At |d| = 0 vtw is NaN in the
        # reference too and neither branch is taken.
        dmin = np.where(slow, 2e-3, 2e-2)
        off_len = dmin + off_len * (0.6 - dmin) / 0.2
        # the fast near envs by thirds: flying toward the waypoint, away from it, as drawn -- both signs of the shaping
        mode = rng.randint(0, 3, n)
        fast = near & ~slow
        speed = np.linalg.norm(fs[3:6], axis=0)
        for m, sign in ((0, 1.0), (1, -1.0)):
            sel = fast & (mode == m)
            fs[3:6, sel] = (sign * speed * off_dir + 0.1 * fs[3:6])[:, sel]
        fs[O.F_FINAL_YAW] = 0.0                           # as the v1 reset leaves it
    else:
        slot = np.where(arrived, K - 1, rng.randint(0, K, n) if K > 1 else 0)
    cur = (tp + off_dir * off_len)
    wps[slot[near], :, cols[near]] = cur[:, near].T
    if v1:
        # final reaches at and past the time limit: the step counter stays and no TRUNCATED bit is set
        last = np.nonzero(near & (off_len < 0.07) & (slot == kep - 1))[0][:3]
        is_[O.I_STEP, last] = ms + np.arange(len(last))
        is_[O.I_FLAGS] = slot | (kep << 4)
    else:
        if K > 1:
            # a few envs about to reach an intermediate waypoint go below z = 0.1, waypoint and all: reach and crash in one step
            sink = np.nonzero(near & ~arrived & (slot < K - 1) & (off_len < 0.08))[0][:4]
            dz = rng.uniform(0.05, 0.085, len(sink)) - fs[2, sink]
            fs[2, sink] += dz; tp[2, sink] += dz; wps[slot[sink], 2, sink] += dz
        is_[O.I_COUNTER] = np.where(arrived, counter, 0)
        is_[O.I_FLAGS] = np.where(arrived, K | O.FLAGBIT_FWR | O.FLAGBIT_COUNTER_ACTIVE, slot)
    fs[O.F_WP0:O.F_WP0 + 3 * K] = wps.reshape(3 * K, n)
    fs[O.F_LAST_DISTANCE] = _apply_last_distance(np.linalg.norm(tp - wps[slot, :, cols].T, axis=0), ld, none_share=0.10)
    return fs, is_


def _last_distance_draws(rng, n):
    u = rng.rand(n)
    wide = rng.uniform(0.04, 0.06, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    tight = rng.normal(0, 0.01, n).clip(-0.02, 0.02)
    return u, wide, tight


def _apply_last_distance(dist, draws, none_share):
    u, wide, tight = draws
    return np.where(u < none_share, -1.0, np.maximum(0.0, np.where(u < none_share + 0.05 * (1 - none_share) / 0.9, dist + tight, dist + wide)))


def _last_distance(dist, rng, none_share):
    """last_distance for envs at distance dist: None (-1) for none_share of them; of the rest 1 in 18 within +-0.02 of dist (around the threshold
    of the +2 progress bonus), the others 0.04..0.06 away on either side: a step travels ~0.005 m, so the oracle's own margin to that
    threshold stays far above the fp32 error and the bonus still goes both ways."""
    return _apply_last_distance(dist, _last_distance_draws(rng, len(dist)), none_share)


def reseat_last_distance(cfg, fstate, rng, istate=None):
    """A copy of fstate with last_distance drawn afresh around each env's present distance, as blob() does (None stays None).  Between the
    steps of a multi-step sweep: the last_distance a step leaves IS the present distance, so that without this every slow env -- every env
    that was just reset above all -- would sit on the threshold of the progress bonus in the next step.  istate: which waypoint is the
    current one (needed with more than one slot)."""
    f = fstate.copy()
    assert istate is not None or (cfg.task.num_waypoints == 1 and not is_v1(cfg))
    wp = f[O.F_WP0:O.F_WP0 + 3] if istate is None else current_waypoint(cfg, f, istate)[0]
    dist = np.linalg.norm(task_point(cfg, f) - wp, axis=0)
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
    configured) with its state after the step under "fstate" / "istate"; post = (fstate, istate, info, obs) of a second oracle WITHOUT
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
    return o, (nr["fstate"], nr["istate"], nr["info"], nr["obs"])


def _rpy(q):
    w, x, y, z = q
    return np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), np.arcsin(np.clip(2 * (w * y - z * x), -1, 1))


def _geometry(cfg, pre, post):
    """Of the step from pre to post: the distance the step measured -- post-step task point to the waypoint that was current BEFORE the
    step (the state machine moves the index after the reward) --, roll, pitch, arrived before the step, last_distance before the step."""
    f0, i0 = pre
    f1 = post[0]
    d = np.linalg.norm(task_point(cfg, f1) - current_waypoint(cfg, f1, i0)[0], axis=0)      # the waypoints stay: post is not reset
    roll, pitch = _rpy(f1[6:10])
    fwr = (i0[O.I_FLAGS] & O.FLAGBIT_FWR) != 0
    return d, roll, pitch, fwr, f0[O.F_LAST_DISTANCE]


def _vtw(cfg, pre, post):
    """v1: the velocity component toward the waypoint, as the reference forms it (NaN at distance 0)."""
    f1 = post[0]
    to_wp = current_waypoint(cfg, f1, pre[1])[0] - f1[0:3]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (f1[3:6] * (to_wp / np.linalg.norm(to_wp, axis=0))).sum(axis=0)


def margins(cfg, pre, post):
    """The oracle's own distance to every threshold the step from pre to post (see oracle_step) can flip, per env; dist is the distance
    to the waypoint that was current before the step.
    v2:
      "info":   min of |dist - 0.1|, |p_z - 0.1|, ||p| - 10|, ||v| - 0.1|, ||w| - 0.1|      (flag bits, and the reward with them)
      "reward": min of those and of the reward-only thresholds: |last_distance - dist| where the progress term counts (last_distance >= 0,
                not arrived before the step), ||roll| - 0.2| and ||pitch| - 0.2| on envs that hold after the step.
    v1:
      "info":   min of |dist - 0.1|, |p_z - 0.1|, ||p| - 10|, ||v| - 0.1|
      "reward": min of those and of ||w| - 0.1|, |dist - 0.5|, |vtw - 0.1| where dist < 0.5, |last_distance - dist| where
                last_distance >= 0."""
    f1 = post[0]
    d, roll, pitch, fwr, ld = _geometry(cfg, pre, post)
    p, v, w = f1[0:3], f1[3:6], f1[10:13]
    inf = np.full(d.shape, np.inf)
    wn = np.abs(np.linalg.norm(w, axis=0) - 0.1)
    info = np.minimum.reduce([np.abs(d - 0.1), np.abs(p[2] - 0.1), np.abs(np.linalg.norm(p, axis=0) - 10), np.abs(np.linalg.norm(v, axis=0) - 0.1)])
    if is_v1(cfg):
        shaping = np.where(d < 0.5, np.nan_to_num(np.abs(_vtw(cfg, pre, post) - 0.1), nan=0.0), inf)
        progress = np.where(ld >= 0, np.abs(ld - d), inf)
        return dict(info=info, reward=np.minimum.reduce([info, wn, np.abs(d - 0.5), shaping, progress]))
    info = np.minimum(info, wn)
    progress = np.where((ld >= 0) & ~fwr, np.abs(ld - d), inf)
    holds = fwr & (d < 0.1)
    tilt = np.where(holds, np.minimum(np.abs(np.abs(roll) - 0.2), np.abs(np.abs(pitch) - 0.2)), inf)
    return dict(info=info, reward=np.minimum.reduce([info, progress, tilt]))


def eligible(m):
    """Envs that `compare` would excuse if they flipped."""
    return m["reward"] < FLIP_MARGIN


def classes(cfg, pre, post, o=None):
    """{class: bool [n]}: the branch of the step state machine each env took in the step from pre to post (oracle_step); the names are
    class_names(cfg).  o (oracle_step's first result, the step WITH auto-reset) is needed on the v1 tasks only: what the reset drew."""
    f1, i1, info, obs = post
    i0 = pre[1]
    d, roll, _, fwr, ld = _geometry(cfg, pre, post)
    bit = lambda b: (info & b) != 0  # noqa: E731
    success, crashed = bit(O.INFO_SUCCESS), bit(O.INFO_CRASHED)
    idx0, idx1 = i0[O.I_FLAGS] & 15, i1[O.I_FLAGS] & 15
    if is_v1(cfg):
        K = (i0[O.I_FLAGS] >> 4) & 15
        vtw = _vtw(cfg, pre, post)
        ended = np.asarray(o["done"]) != 0
        drew = (np.asarray(o["istate"])[O.I_FLAGS] >> 4) & 15
        return dict(truncated=bit(O.INFO_TRUNCATED), crashed_sinking=crashed & (f1[5] < 0), crashed_rising=crashed & (f1[5] >= 0), oob=bit(O.INFO_OOB),
                    intermediate_reach=(idx1 == idx0 + 1) & ~success, final_reach_stopped=success & bit(O.INFO_STOPPED),
                    final_reach_moving=success & ~bit(O.INFO_STOPPED),
                    final_reach_at_time_limit=success & (i0[O.I_STEP] >= cfg.task.max_episode_steps) & (i1[O.I_STEP] == i0[O.I_STEP]) & ~bit(O.INFO_TRUNCATED),
                    shaping_plus=(d < 0.5) & (vtw > 0.1), shaping_minus=(d < 0.5) & (vtw < 0.1), shaping_off=~(d < 0.5),
                    progress_taken=(ld >= 0) & (ld - d > 0), progress_not_taken=(ld >= 0) & (ld - d <= 0), last_distance_none=ld < 0,
                    is_final_0=(obs[:, 16] == 0) & (idx1 < K - 1), is_final_1=(obs[:, 16] == 1) & (idx1 >= K - 1),
                    reset_drew_k1=ended & (drew == 1), reset_drew_k2=ended & (drew == 2))
    counts = (ld >= 0) & ~fwr
    c = dict(truncated=bit(O.INFO_TRUNCATED), crashed_sinking=crashed & (f1[5] < 0), crashed_rising=crashed & (f1[5] >= 0), oob=bit(O.INFO_OOB),
             first_arrival=success & ~fwr, hold_level=success & fwr & (np.abs(roll) < 0.2), hold_tilted=success & fwr & (np.abs(roll) >= 0.2),
             stopped=bit(O.INFO_STOPPED), hold_terminated=success & bit(O.INFO_TERMINATED), arrived_outside=fwr & ~success,
             progress_taken=counts & (ld - d > 0), progress_not_taken=counts & (ld - d <= 0), last_distance_none=ld < 0)
    K = cfg.task.num_waypoints
    if K > 1:
        reach = (idx1 == idx0 + 1) & ~success
        nxt = (obs[:, 16:19] != 0).any(axis=1)
        c.update(intermediate_reach=reach, intermediate_reach_then_crash_or_oob=reach & (crashed | bit(O.INFO_OOB)),
                 final_first_arrival=success & ~fwr & (idx0 == K - 1) & (idx1 == K),
                 next_waypoint_columns_nonzero=(idx1 < K - 1) & nxt, next_waypoint_columns_zero=(idx1 >= K - 1) & ~nxt)
    return c


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _worst(x):
    return float(x.max()) if x.size else 0.0


def compare(g, o, m, dtype, flags=O.FLAG_AUTO_RESET):
    """Assert that one step of the kernels (g) is the oracle's (o: oracle_step's first result) within the gates at the top of this file,
    m = margins(...) of that step, flags the handle's flag word.  Both hold obs, reward, done, info, terminal_obs, ep_return, ep_len of the
    step and the state after it under "fstate" / "istate"; rows of terminal_obs / ep_return / ep_len must have been NaN / NaN / -1 before
    the step (the oracle binding does that itself).  Returns the flip count, the flipped envs and the worst error of every gated quantity."""
    f32 = dtype == "f32"
    auto = (flags & O.FLAG_AUTO_RESET) != 0
    n = len(o["done"])
    gi, oi = np.asarray(g["info"]).view(np.uint32), np.asarray(o["info"]).view(np.uint32)
    gr, orw = np.asarray(g["reward"], np.float64), np.asarray(o["reward"], np.float64)
    gf, of = np.asarray(g["fstate"], np.float64), np.asarray(o["fstate"], np.float64)
    # ---- NONFINITE envs (either side says so): never a flip; every flag bit equal, reward exactly -100
    nf = ((gi | oi) & O.INFO_NONFINITE) != 0
    assert (flags & O.FLAG_NAN_GUARD) or not nf.any(), ("NONFINITE without the guard", np.nonzero(nf)[0][:8])
    bad = nf & (gi != oi)
    assert not bad.any(), ("flag bits of NONFINITE envs", np.nonzero(bad)[0][:8], gi[bad][:8], oi[bad][:8])
    assert (gr[nf] == -100.0).all() and (orw[nf] == -100.0).all(), ("reward of NONFINITE envs", gr[nf][:8])
    with np.errstate(invalid="ignore"):
        e_rew = np.abs(gr - orw) / np.maximum(1.0, np.abs(orw))
    flip_info = ~nf & ((gi & 127) != (oi & 127))
    flip_rew = ~nf & ~flip_info & ~(e_rew < (REW32 if f32 else REW64))
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
    # envs whose state the step leaves (all that were not reset; a NONFINITE env's float state is unspecified), envs that were reset, envs that ended
    on, reset, ended = ok & ~(done & auto) & ~nf, ok & done & auto, ok & done
    e_state = np.abs(gf - of)[:, on] if not f32 else rel_err(gf, of)[:, on]
    assert _worst(e_state) < (REL32 if f32 else ABS64) and not np.isnan(e_state).any(), ("state of envs that go on: worst per row", e_state.max(axis=1))
    assert np.array_equal(gf[:, reset], of[:, reset]), "reset states are bit-equal"
    go, oo = np.asarray(g["obs"], np.float64), np.asarray(o["obs"], np.float64)
    obs_err = (lambda a, b: rel_err(a, b)) if f32 else (lambda a, b: np.abs(a - b))
    obs_gate = REL32 if f32 else OBS64
    rows = ok & ~(nf & (not auto))                                    # (a NONFINITE env that is not reset: the row is its terminal row)
    e_obs = obs_err(go[rows], oo[rows])
    assert _worst(e_obs) < obs_gate and not np.isnan(e_obs).any(), ("observation rows", _worst(e_obs))
    # ---- envs that ended, and the rows of those that did not
    was_reset = (gi & O.INFO_WAS_RESET) != 0
    assert np.array_equal(was_reset[ok], (oi[ok] & O.INFO_WAS_RESET) != 0) and np.array_equal(was_reset[ok], reset[ok]), "INFO_WAS_RESET"
    assert np.array_equal(np.asarray(g["ep_len"])[ended], np.asarray(o["ep_len"])[ended]), "ep_len"
    ret = ended & np.isfinite(np.asarray(o["ep_return"], np.float64))        # (a non-finite running return with finite state: out of scope)
    assert not (ended & ~ret & ~nf).any(), "the oracle's ep_return of a finite env is not finite"
    e_ret = rel_err(np.asarray(g["ep_return"])[ret], np.asarray(o["ep_return"])[ret])
    assert _worst(e_ret) < RET_REL and not np.isnan(e_ret).any(), ("ep_return", _worst(e_ret))
    trows = ended & ~nf
    e_tobs = obs_err(np.asarray(g["terminal_obs"], np.float64)[trows], np.asarray(o["terminal_obs"], np.float64)[trows])
    assert _worst(e_tobs) < obs_gate and not np.isnan(e_tobs).any(), ("terminal rows", _worst(e_tobs))
    kept = np.asarray(g["done"]) == 0
    assert np.isnan(np.asarray(g["terminal_obs"])[kept]).all() and np.isnan(np.asarray(g["ep_return"])[kept]).all() and (np.asarray(g["ep_len"])[kept] == -1).all(), \
        "rows of envs that did not end were written"
    return dict(flips=int(flips.sum()), flipped=np.nonzero(flips)[0], ended=int(ended.sum()), nonfinite=int(nf.sum()), state=_worst(e_state), reward=_worst(e_rew[ok & ~nf]),
                obs=_worst(e_obs), ep_return=_worst(e_ret), terminal_obs=_worst(e_tobs))
