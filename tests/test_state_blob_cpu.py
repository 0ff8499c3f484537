"""The oracle alone on the states of tests/test_gpu_branch_sweep.py: what that sweep relies on, checked where no GPU is needed.

  1. Branch coverage: the blob of tests/state_blob.py reaches every branch of the step state machine on every vehicle, batch size and seed
     the sweep uses -- at least 8 envs per branch in the first step of the 4100-env case, at least one over the six steps of a 300-env case
     (and a hold-phase env and a hold termination within the four steps its rollout cases run).
  2. The cap on threshold flips is a condition, not a measurement: in every step the envs the comparison WOULD excuse (oracle margin below
     3e-5) number at most the cap, so a disagreement beyond them cannot hide behind it.
  3. `compare` accepts the oracle against itself and rejects a copy changed in any one field it guards.
  4. The same for the states of the other two task forms (TASK_STATES: v1, and v2 with 2..4 waypoints), with the classes of those tasks; and
     the one-waypoint states are still, by checksum, the ones the sweep started from before the blob learnt the other tasks.
  5. Conditions 1 and 2 on the fully general vehicles and task constants of tests/generic_vehicles.py (GENERIC_STATES, GENERIC_TASK_STATES:
     what tests/test_gpu_generic_vehicles.py starts from); if a parameter set misses one, the parameters change, not the cap."""
import copy
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from tests import generic_vehicles as GV
from tests import state_blob as B
from tests.test_arm_cpu import arm_cfg

BLOB_SEED, ACTION_SEED, RESEAT_SEED, ENV_SEED = 11, 12, 13, 21
STEPS, ROLLOUT_STEPS = 6, 4
# (vehicle, n, dtype) of every state the sweep starts from
STATES = [("hexa_arm", 300, "f32"), ("hexa_arm", 300, "f64"), ("hexa_arm", 4100, "f32"), ("hexa_arm_2j", 300, "f32"), ("hexa_arm_base", 300, "f32"),
          ("hexa", 300, "f32"), ("hexa", 300, "f64"), ("quad", 300, "f32")]
# the fully general vehicles of tests/generic_vehicles.py on its task constants (tests/test_gpu_generic_vehicles.py starts from these)
GENERIC_STATES = [("gen_arm", 300, "f32"), ("gen_arm", 300, "f64"), ("gen_arm_2j", 300, "f32"), ("gen_arm_base", 300, "f32"), ("gen_arm_yzx", 300, "f32"),
                  ("gen_arm_yzx", 300, "f64"), ("gen_arm_skew", 300, "f32"), ("gen_arm_skew", 300, "f64"), ("gen_quad", 300, "f32"), ("gen_quad", 300, "f64"),
                  ("gen_hexa", 300, "f32"), ("gen_hexa", 300, "f64")]
GENERIC_TASK_STATES = [("gen_quad", 300, "f32", "v1_raw"), ("gen_hexa", 300, "f32", "v2k3"), ("gen_arm", 300, "f32", "v2k3")]


# The other two task forms the kernels are built in (KW = 4 on v2, KW = 2 on v1): (vehicle, n, dtype, task) of every state the sweep's cases
# for them start from.  task: "v2" (one waypoint, the states above), "v2k2".."v2k4", "v1_raw", "v1_scaled"
TASK_STATES = [("quad", 300, "f32", "v1_raw"), ("quad", 300, "f64", "v1_raw"), ("quad", 300, "f32", "v1_scaled"), ("hexa", 300, "f32", "v1_scaled"),
               ("quad", 300, "f32", "v2k3"), ("quad", 300, "f64", "v2k3"), ("hexa", 300, "f32", "v2k4"), ("hexa", 300, "f32", "v2k2"),
               ("hexa", 300, "f32", "v2k3"), ("hexa_arm", 300, "f32", "v2k3"), ("hexa_arm", 300, "f64", "v2k3"), ("hexa_arm_2j", 300, "f32", "v2k2")]
V1_VARIANT = {"v1_scaled": O.TASK_V1_SCALED17, "v1_raw": O.TASK_V1_RAW17}
# zlib.crc32(fstate.tobytes() + istate.tobytes()) of every entry of STATES, taken before blob() learnt the other tasks: the one-waypoint
# sweep still starts from the same states
STATE_CRC = {("hexa_arm", 300, "f32"): 0x180aced9, ("hexa_arm", 300, "f64"): 0xf453e011, ("hexa_arm", 4100, "f32"): 0x483d7431,
             ("hexa_arm_2j", 300, "f32"): 0x81c8b385, ("hexa_arm_base", 300, "f32"): 0x9d8d7d3f, ("hexa", 300, "f32"): 0x8fdd3bde,
             ("hexa", 300, "f64"): 0x6aa8787a, ("quad", 300, "f32"): 0x8fdd3bde}       # (a rigid vehicle's blob does not depend on its rotors)


def oracle_cfg(vehicle, n, task="v2"):
    """The oracle's config of a sweep vehicle: the package's vehicle parameters on the reference task, auto-reset on; a "gen_..." vehicle:
    tests/generic_vehicles.py's parameters and task constants in their place."""
    if vehicle in GV.VEHICLES:
        cfg = oracle_cfg({"gen_quad": "quad", "gen_hexa": "hexa"}.get(vehicle, "hexa_arm"), n, task)
        return GV.build(cfg, vehicle)
    if task != "v2":
        veh = oracle_cfg(vehicle, n)
        if task in V1_VARIANT:
            cfg = O.reference_quad_config(1, variant=V1_VARIANT[task])
        else:
            cfg = O.reference_quad_config(1, num_waypoints=int(task[3:]))
        C.memmove(C.byref(cfg.vehicle), C.byref(veh.vehicle), C.sizeof(O.Vehicle))
        cfg.task.ee_task = veh.task.ee_task
        cfg.num_envs, cfg.seed, cfg.flags = n, ENV_SEED, O.FLAG_AUTO_RESET
        return cfg
    if vehicle.startswith("hexa_arm"):
        if vehicle == "hexa_arm_2j":
            cfg = arm_cfg(n_joints=2, mass=amd._lib.default_config("hexa_arm", 1, n_joints=2).vehicle.mass)
        else:
            cfg = arm_cfg()
        if vehicle == "hexa_arm_base":
            cfg.task.ee_task = O.EE_TASK_BASE
    else:
        cfg = O.reference_quad_config(1)
        if vehicle == "hexa":
            C.memmove(C.byref(cfg.vehicle), C.byref(amd._lib.default_config("hexa", 1).vehicle), C.sizeof(O.Vehicle))
    cfg.num_envs, cfg.seed, cfg.flags = n, ENV_SEED, O.FLAG_AUTO_RESET
    return cfg


@functools.lru_cache(maxsize=None)
def start_state(vehicle, n, dtype, task="v2"):
    """(cfg, fstate, istate): the blob of this vehicle, batch size and task as a handle of dtype holds it.  Shared: do not write to it."""
    cfg = oracle_cfg(vehicle, n, task)
    fs, is_ = B.blob(cfg, n, np.random.RandomState(BLOB_SEED))
    if dtype == "f32":
        fs = B.to_f32(fs)
    fs.setflags(write=False); is_.setflags(write=False)
    return cfg, fs, is_


@functools.lru_cache(maxsize=None)
def oracle_run(vehicle, n, dtype, task="v2"):
    """STEPS steps of the oracle alone, as the sweep runs them (last_distance drawn afresh between the steps): per step (pre, actions, o, post)."""
    cfg, fs, is_ = start_state(vehicle, n, dtype, task)
    rng, rng_ld = np.random.RandomState(ACTION_SEED), np.random.RandomState(RESEAT_SEED)
    pre, run = (fs, is_), []
    for t in range(STEPS):
        a = B.actions(cfg, pre[0], rng)
        o, post = B.oracle_step(cfg, pre, a)
        run.append((pre, a, o, post))
        f = B.reseat_last_distance(cfg, o["fstate"], rng_ld, o["istate"])
        pre = (B.to_f32(f) if dtype == "f32" else f, o["istate"])
    return cfg, run


@pytest.mark.parametrize("vehicle,n,dtype", STATES + GENERIC_STATES)
def test_blob_reaches_every_branch_and_the_flip_cap_is_a_condition(vehicle, n, dtype):
    cfg, run = oracle_run(vehicle, n, dtype)
    per_step = []
    for t, (pre, a, o, post) in enumerate(run):
        m = B.margins(cfg, pre, post)
        n_el = int(B.eligible(m).sum())
        assert n_el <= B.flip_cap(n), f"step {t}: {n_el} envs within {B.FLIP_MARGIN} of a threshold, the cap is {B.flip_cap(n)}"
        per_step.append({k: int(v.sum()) for k, v in B.classes(cfg, pre, post).items()})
        print(f"{vehicle} n={n} {dtype} step {t}: eligible {n_el}", per_step[-1])
    assert set(per_step[0]) == set(B.CLASSES)
    over = {k: sum(c[k] for c in per_step) for k in B.CLASSES}
    assert all(over[k] >= 1 for k in B.CLASSES), over
    if n >= 4096:
        assert all(per_step[0][k] >= 8 for k in B.CLASSES), per_step[0]
    head = {k: sum(c[k] for c in per_step[:ROLLOUT_STEPS]) for k in B.CLASSES}
    assert per_step[0]["hold_level"] + per_step[0]["hold_tilted"] >= 1 and head["hold_terminated"] >= 1, head


def test_one_waypoint_states_are_the_ones_the_sweep_always_ran():
    assert set(STATE_CRC) == set(STATES)
    for key in STATES:
        _, fs, is_ = start_state(*key)
        assert zlib.crc32(fs.tobytes() + is_.tobytes()) == STATE_CRC[key], key


@pytest.mark.parametrize("vehicle,n,dtype,task", TASK_STATES + GENERIC_TASK_STATES)
def test_task_blob_reaches_every_branch_and_the_flip_cap_is_a_condition(vehicle, n, dtype, task):
    """The same two conditions on the states of the v1 and the multi-waypoint cases: every class of the task within the six steps (what the
    rollout cases rely on within theirs), and in every step no more envs within FLIP_MARGIN of a threshold than the cap."""
    cfg, run = oracle_run(vehicle, n, dtype, task)
    names = B.class_names(cfg)
    per_step = []
    for t, (pre, a, o, post) in enumerate(run):
        m = B.margins(cfg, pre, post)
        n_el = int(B.eligible(m).sum())
        assert n_el <= B.flip_cap(n), f"step {t}: {n_el} envs within {B.FLIP_MARGIN} of a threshold, the cap is {B.flip_cap(n)}"
        per_step.append({k: int(v.sum()) for k, v in B.classes(cfg, pre, post, o).items()})
        print(f"{vehicle} {task} n={n} {dtype} step {t}: eligible {n_el}", per_step[-1])
    assert set(per_step[0]) == set(names)
    over = {k: sum(c[k] for c in per_step) for k in names}
    assert all(over[k] >= 1 for k in names), over
    head = {k: sum(c[k] for c in per_step[:ROLLOUT_STEPS]) for k in names}
    ended_early = sum(int((o["done"] != 0).sum()) for _, _, o, _ in run[:ROLLOUT_STEPS - 1])
    assert head["intermediate_reach"] >= 1 and ended_early >= 1, head
    if task in V1_VARIANT:
        assert head["final_reach_stopped"] + head["final_reach_moving"] >= 1 and head["final_reach_at_time_limit"] >= 1, head
        assert head["reset_drew_k1"] >= 1 and head["reset_drew_k2"] >= 1, head
    else:
        assert per_step[0]["hold_level"] + per_step[0]["hold_tilted"] >= 1 and head["hold_terminated"] >= 1, head
        assert head["final_first_arrival"] >= 1 and head["intermediate_reach_then_crash_or_oob"] >= 1, head


def test_task_blobs_hold_what_their_tasks_store():
    cfg, fs, is_ = start_state("quad", 300, "f32", "v1_raw")
    fl = is_[O.I_FLAGS]
    kep, idx = (fl >> 4) & 15, fl & 15
    assert fs.shape == (22, 300) and set(kep) == {1, 2} and (idx < kep).all() and (fl >> 8 == 0).all() and (is_[O.I_COUNTER] == 0).all()
    assert (fs[19:22, kep == 1] == 0).all() and (fs[19:22, kep == 2] != 0).all() and set(idx[kep == 2]) == {0, 1}
    d = np.linalg.norm(fs[0:3] - B.current_waypoint(cfg, fs, is_)[0], axis=0)
    assert d.min() > 1e-3 and (d < 0.1).sum() > 5 and ((d > 0.1) & (d < 0.5)).sum() > 20 and ((d > 0.5) & (d < 0.6)).sum() > 5
    ms = cfg.task.max_episode_steps
    assert ms == 1200 and ((d < 0.1) & (idx == kep - 1) & (is_[O.I_STEP] >= ms)).sum() >= 2 and (is_[O.I_STEP] < ms).any()
    for vehicle, task, K, nf in (("quad", "v2k3", 3, 25), ("hexa", "v2k4", 4, 28), ("hexa_arm", "v2k3", 3, 31), ("hexa_arm_2j", "v2k2", 2, 26)):
        cfg, fs, is_ = start_state(vehicle, 300, "f32", task)
        fl = is_[O.I_FLAGS]
        arrived = (fl & O.FLAGBIT_FWR) != 0
        assert fs.shape == (nf, 300) and (fs[16:nf] != 0).all()
        assert ((fl[arrived] & 1023) == (K | O.FLAGBIT_FWR | O.FLAGBIT_COUNTER_ACTIVE)).all() and set(fl[~arrived]) == set(range(K))


def test_blob_fills_every_field_of_a_shorter_arm():
    cfg, fs, is_ = start_state("hexa_arm_2j", 300, "f32")
    assert fs.shape == (23, 300) and (fs[19:23] != 0).all() and np.abs(fs[20]).max() <= 1.5 and np.abs(fs[19]).max() > 1.5
    cfg, fs, is_ = start_state("hexa_arm", 300, "f32")
    assert fs.shape == (25, 300) and (fs[19:25] != 0).all()
    cfg, fs, is_ = start_state("quad", 300, "f32")
    assert fs.shape == (19, 300)
    arrived = (is_[O.I_FLAGS] & O.FLAGBIT_FWR) != 0
    assert ((is_[O.I_FLAGS][arrived] & 255) == 1).all() and (is_[O.I_COUNTER][~arrived] == 0).all() and is_[O.I_COUNTER].max() > cfg.task.counter_limit
    assert is_[O.I_STEP].max() > cfg.task.max_episode_steps


# ---- compare() itself ----------------------------------------------------------------------------------------------------------------------
def _first_step():
    cfg, run = oracle_run("hexa_arm", 300, "f32")
    pre, a, o, post = run[0]
    return o, B.margins(cfg, pre, post)


def _pick(mask):
    k = np.nonzero(mask)[0]
    assert len(k), "the self-test needs such an env"
    return int(k[0])


def test_compare_accepts_the_oracle_against_itself():
    o, m = _first_step()
    for dtype in ("f32", "f64"):
        r = B.compare(copy.deepcopy(o), o, m, dtype)
        assert r["flips"] == 0 and r["ended"] > 10 and max(r["state"], r["reward"], r["obs"], r["ep_return"], r["terminal_obs"]) == 0.0


def _change(field):
    """A copy of the oracle's first step changed in one field, on an env far from every threshold."""
    o, m = _first_step()
    g = copy.deepcopy(o)
    clear = m["reward"] > 1e-2
    done = o["done"] != 0
    if field == "reward":
        g["reward"][_pick(clear & (np.abs(o["reward"]) < 10))] += 1e-3
    elif field == "info":
        g["info"][_pick(clear)] ^= O.INFO_STOPPED
    elif field == "ep_len":
        g["ep_len"][_pick(done)] += 1
    elif field == "terminal_obs":
        g["terminal_obs"][_pick(done), 3] += 1e-3
    elif field == "int field":
        g["istate"][O.I_COUNTER, _pick(clear & ~done)] += 1
    elif field == "ep_return":
        k = _pick(done)
        g["ep_return"][k] += 1e-3 * max(1.0, abs(g["ep_return"][k]))
    elif field == "running return":
        k = _pick(clear & ~done)
        g["fstate"][O.F_EP_RETURN, k] += 1e-3 * max(1.0, abs(g["fstate"][O.F_EP_RETURN, k]))
    elif field == "last_distance":
        g["fstate"][O.F_LAST_DISTANCE, _pick(clear & ~done)] += 1e-4
    elif field == "reset state":
        g["fstate"][0, _pick(done)] += 1e-7
    elif field == "observation":
        g["obs"][_pick(clear), 28] += 1e-4
    elif field == "was_reset":
        g["info"][_pick(done)] &= ~np.uint32(O.INFO_WAS_RESET)
    elif field == "row of an env that did not end":
        g["ep_len"][_pick(~done)] = 7
    elif field == "terminal row of an env that did not end":
        g["terminal_obs"][_pick(~done), 0] = 0.0
    elif field == "done":
        g["done"][_pick(clear & ~done)] = 1
    else:
        raise KeyError(field)
    return g, o, m


@pytest.mark.parametrize("field", ["reward", "info", "ep_len", "terminal_obs", "int field", "ep_return", "running return", "last_distance", "reset state",
                                   "observation", "was_reset", "row of an env that did not end", "terminal row of an env that did not end", "done"])
def test_compare_rejects_one_changed_field(field):
    g, o, m = _change(field)
    with pytest.raises(AssertionError):
        B.compare(g, o, m, "f32")


def test_compare_excuses_a_flip_only_on_a_threshold_and_only_up_to_the_cap():
    o, m = _first_step()
    g = copy.deepcopy(o)
    ks = np.nonzero((m["reward"] > 1e-2) & (o["done"] == 0))[0][:2]
    g["info"][ks[0]] ^= O.INFO_STOPPED
    on_threshold = {k: v.copy() for k, v in m.items()}
    on_threshold["info"][ks] = 1e-6; on_threshold["reward"][ks] = 1e-6
    r = B.compare(g, o, on_threshold, "f32")
    assert r["flips"] == 1 and list(r["flipped"]) == [ks[0]]
    with pytest.raises(AssertionError):            # the fp64 builds take every comparison as the oracle does
        B.compare(g, o, on_threshold, "f64")
    g["reward"][ks[1]] += 2.0                      # a second one: 300 envs allow one
    with pytest.raises(AssertionError):
        B.compare(g, o, on_threshold, "f32")


# ---- compare() on a step of the v1 state machine ---------------------------------------------------------------------------------------------
def _v1_step():
    cfg, run = oracle_run("quad", 300, "f32", "v1_raw")
    pre, a, o, post = run[0]
    return o, B.margins(cfg, pre, post)


def test_compare_accepts_a_v1_step_of_the_oracle_against_itself():
    o, m = _v1_step()
    for dtype in ("f32", "f64"):
        r = B.compare(copy.deepcopy(o), o, m, dtype)
        assert r["flips"] == 0 and r["ended"] > 10 and max(r["state"], r["reward"], r["obs"], r["ep_return"], r["terminal_obs"]) == 0.0


@pytest.mark.parametrize("field", ["is_final column", "waypoint count of an env that goes on", "shaping-sized reward error"])
def test_compare_rejects_one_changed_field_of_a_v1_step(field):
    o, m = _v1_step()
    g = copy.deepcopy(o)
    clear = m["reward"] > 1e-2
    on = o["done"] == 0
    if field == "is_final column":
        k = _pick(clear)
        g["obs"][k, 16] = 1.0 - g["obs"][k, 16]
    elif field == "waypoint count of an env that goes on":
        g["istate"][O.I_FLAGS, _pick(clear & on)] ^= 0x30          # flag bits 4-7: one waypoint <-> two
    else:
        g["reward"][_pick(clear & on)] -= 10.0
    for dtype in ("f32", "f64"):
        with pytest.raises(AssertionError):
            B.compare(g, o, m, dtype)


# ---- the flag word: NaN guard and auto-reset off (tests/test_gpu_flag_sweep.py) ----------------------------------------------------------------
POISON_SEED = 14
GUARD_AUTO, GUARD, PLAIN = O.FLAG_NAN_GUARD | O.FLAG_AUTO_RESET, O.FLAG_NAN_GUARD, 0
FLAG_WORDS = {"guard_auto": GUARD_AUTO, "guard": GUARD, "plain": PLAIN}
ACTION_POISON_STEPS = (0, 3)


def flag_n(vehicle, n):
    """The batch size of a flag-sweep case: the 3-joint arm poisons 78 envs (57 state, 21 action), a quarter of 312, so it runs at 600."""
    return max(n, 600) if vehicle in ("hexa_arm", "hexa_arm_base") else n


# every (vehicle, n, dtype, task) the flag sweep starts from: the states of both branch sweeps at flag_n
FLAG_STATES = sorted({(v, flag_n(v, n), d, "v2") for v, n, d in STATES} | {(v, flag_n(v, n), d, t) for v, n, d, t in TASK_STATES})


@functools.lru_cache(maxsize=None)
def poisoned_start(vehicle, n, dtype, task="v2"):
    """(cfg, fstate, istate, masks): start_state with B.poison's state poison in it.  Envs the branch classes need (the first three of every
    class in the clean oracle run) are left alone; one env at the time limit, one in the hold phase and one about to reach its waypoint in
    the first step are among the poisoned ones.  Shared: do not write to it."""
    cfg, fs, is_ = start_state(vehicle, n, dtype, task)
    _, run = oracle_run(vehicle, n, dtype, task)
    avoid = np.zeros(n, bool)
    for name in B.class_names(cfg):
        hits = np.concatenate([np.nonzero(B.classes(cfg, pre, post, o)[name])[0] for pre, _, o, post in run])
        avoid[list(dict.fromkeys(hits.tolist()))[:3]] = True
    pre, _, o, post = run[0]
    d, _, _, fwr, _ = B._geometry(cfg, pre, post)
    late = pre[1][O.I_STEP] >= cfg.task.max_episode_steps
    wanted = [late & ~avoid, (d < 0.1) & ~fwr & ~late & ~avoid] + ([] if B.is_v1(cfg) else [fwr & (d < 0.1) & ~late & ~avoid])
    must = [int(np.nonzero(w)[0][-1]) for w in wanted]
    f, _, masks = B.poison(cfg, fs, np.zeros((n, 4 + cfg.vehicle.n_joints), np.float32), np.random.RandomState(POISON_SEED), must=must, avoid=avoid)
    f.setflags(write=False)
    return cfg, f, is_, masks


def flag_actions(cfg, pre, rng, t, masks):
    """Step t's actions of a flag-sweep case: B.actions, with the action poison on ACTION_POISON_STEPS when the blob is the poisoned one."""
    a = B.actions(cfg, pre[0], rng)
    return B.poison_actions(a, masks) if masks is not None and t in ACTION_POISON_STEPS else a


@functools.lru_cache(maxsize=None)
def flag_run(vehicle, n, dtype, task, flags):
    """STEPS steps of the oracle alone as the flag sweep runs them: with the guard from the poisoned blob, else from the clean one; beside
    it the clean twin (guard off, clean blob, same auto-reset).  Per step (pre, actions, o, post, clean_distance, twin's o)."""
    guard = (flags & O.FLAG_NAN_GUARD) != 0
    cfg, fs, is_, masks = poisoned_start(vehicle, n, dtype, task) if guard else start_state(vehicle, n, dtype, task) + (None,)
    cfg = B._cfg_for(cfg, n, flags)
    tcfg = B._cfg_for(cfg, n, flags & ~O.FLAG_NAN_GUARD)
    rngs = [(np.random.RandomState(ACTION_SEED), np.random.RandomState(RESEAT_SEED)) for _ in range(2)]
    pre, tpre, run = (fs, is_), start_state(vehicle, n, dtype, task)[1:], []
    for t in range(STEPS):
        a, ta = flag_actions(cfg, pre, rngs[0][0], t, masks), flag_actions(tcfg, tpre, rngs[1][0], t, None)
        (o, post), (to, tpost) = B.oracle_step(cfg, pre, a), B.oracle_step(tcfg, tpre, ta)
        run.append((pre, a, o, post, B._geometry(tcfg, tpre, tpost)[0], to))
        nxt = []
        for c, oo, (_, rl) in ((cfg, o, rngs[0]), (tcfg, to, rngs[1])):
            with np.errstate(invalid="ignore"):
                f = B.reseat_last_distance(c, oo["fstate"], rl, oo["istate"])
            nxt.append((B.to_f32(f) if dtype == "f32" else f, oo["istate"]))
        pre, tpre = nxt
    return cfg, masks, run


@pytest.mark.parametrize("word", list(FLAG_WORDS))
@pytest.mark.parametrize("vehicle,n,dtype,task", FLAG_STATES)
def test_flag_runs_reach_every_class_on_the_oracle(vehicle, n, dtype, task, word):
    """What tests/test_gpu_flag_sweep.py relies on: the poison stays below a quarter of the batch and leaves every branch class reached on
    the clean envs; every class of the guard is reached; the clean envs are, bit for bit, those of the clean twin; the flip cap is still a
    condition; `compare` accepts each step against itself."""
    flags = FLAG_WORDS[word]
    cfg, masks, run = flag_run(vehicle, n, dtype, task, flags)
    guard, auto = (flags & O.FLAG_NAN_GUARD) != 0, (flags & O.FLAG_AUTO_RESET) != 0
    clean = masks["clean"] if guard else np.ones(n, bool)
    names = [k for k in B.class_names(cfg) if auto or not k.startswith("reset_drew")]       # (what a reset drew: there is none without auto-reset)
    seen, seen_nf = {k: 0 for k in names}, {k: 0 for k in B.nonfinite_class_names(cfg)}
    if guard:
        n_s, n_a = 3 * len(B.guarded_rows(cfg)), 3 * (4 + cfg.vehicle.n_joints)
        assert int(masks["state"].sum()) == n_s and int(masks["action"].sum()) == n_a and n_s + n_a <= 0.25 * n
        assert all(masks["state"][e] for e in (0, 15, 16, 63, 64, n - 1))
    for t, (pre, a, o, post, clean_d, to) in enumerate(run):
        with np.errstate(invalid="ignore"):
            m = B.margins(cfg, pre, post)
            cl = B.classes(cfg, pre, post, o)
        n_el = int(B.eligible(m).sum())
        assert n_el <= B.flip_cap(n), f"step {t}: {n_el} envs within {B.FLIP_MARGIN} of a threshold, the cap is {B.flip_cap(n)}"
        for k in names:
            seen[k] += int((cl[k] & clean).sum())
        nf = (o["info"] & O.INFO_NONFINITE) != 0
        assert not nf[clean].any()
        for k in ("obs", "reward", "done", "info"):                      # isolation, on the oracle: a clean env does not see the poison
            assert np.array_equal(np.asarray(o[k])[clean], np.asarray(to[k])[clean]), (t, k)
        assert np.array_equal(o["fstate"][:, clean], to["fstate"][:, clean]) and np.array_equal(o["istate"][:, clean], to["istate"][:, clean]), t
        if guard:
            for k, v in B.nonfinite_classes(cfg, pre, a, o["info"], clean_d).items():
                seen_nf[k] += int(v.sum())
            if t == 0 or not auto:
                assert nf[masks["state"]].all(), (t, "state poison not flagged", np.nonzero(masks["state"] & ~nf)[0])
            # action poison: flagged on its steps; between them only an env whose state it reached (a NaN joint command, never reset)
            stale = ~np.isfinite(pre[0][B.guarded_rows(cfg)]).all(axis=0)
            assert not (auto and stale[masks["action"]].any())
            assert np.array_equal(nf[masks["action"]], np.ones(int(masks["action"].sum()), bool) if t in ACTION_POISON_STEPS else stale[masks["action"]]), t
            assert (o["reward"][nf] == -100.0).all() and ((o["info"][nf] & O.INFO_TERMINATED) != 0).all() and (o["done"][nf] == 1).all()
        with np.errstate(invalid="ignore"):
            r = B.compare(copy.deepcopy(o), o, m, dtype, flags)
        assert r["flips"] == 0 and r["nonfinite"] == int(nf.sum())
    print(vehicle, task, n, dtype, word, seen, seen_nf)
    assert all(v >= 1 for v in seen.values()), seen
    assert not guard or all(v >= 1 for v in seen_nf.values()), seen_nf


@pytest.mark.parametrize("vehicle,n,dtype,task", [s for s in FLAG_STATES if s[2] == "f32" and s[1] < 4096])
def test_guard_on_is_bit_equal_to_guard_off_on_the_clean_blob(vehicle, n, dtype, task):
    cfg, fs, is_ = start_state(vehicle, n, dtype, task)
    a = B.actions(cfg, fs, np.random.RandomState(ACTION_SEED))
    for auto in (O.FLAG_AUTO_RESET, 0):
        on, _ = B.oracle_step(B._cfg_for(cfg, n, auto | O.FLAG_NAN_GUARD), (fs, is_), a)
        off, _ = B.oracle_step(B._cfg_for(cfg, n, auto), (fs, is_), a)
        for k in on:
            assert np.array_equal(np.asarray(on[k]), np.asarray(off[k]), equal_nan=True), k


def _guard_step():
    cfg, masks, run = flag_run("quad", 300, "f32", "v2", GUARD_AUTO)
    pre, a, o, post, _, _ = run[0]
    with np.errstate(invalid="ignore"):
        return o, B.margins(cfg, pre, post), masks


@pytest.mark.parametrize("field", ["flag bits", "reward", "int field", "ep_len", "ep_return", "reset state", "post-reset row", "missed", "invented"])
def test_compare_rejects_one_changed_field_of_a_nonfinite_env(field):
    """A NONFINITE env is never an excusable flip, whatever the margins say, and is gated on everything but its terminal row."""
    o, m, masks = _guard_step()
    g = copy.deepcopy(o)
    k = int(masks["state_env"][0])
    assert o["info"][k] & O.INFO_NONFINITE
    m = {q: np.full_like(v, 1e-9) for q, v in m.items()}              # every env "on a threshold"
    if field == "flag bits":
        g["info"][k] |= O.INFO_TRUNCATED
    elif field == "reward":
        g["reward"][k] = np.nextafter(-100.0, 0.0)
    elif field == "int field":
        g["istate"][O.I_EPISODE, k] += 1
    elif field == "ep_len":
        g["ep_len"][k] += 1
    elif field == "ep_return":
        g["ep_return"][k] += 1e-3 * max(1.0, abs(g["ep_return"][k]))
    elif field == "reset state":
        g["fstate"][0, k] += 1e-7
    elif field == "post-reset row":
        g["obs"][k, 2] += 1e-4
    elif field == "missed":
        g["info"][k] &= ~np.uint32(O.INFO_NONFINITE)
    else:
        j = _pick(masks["clean"] & (o["done"] == 0))
        g["info"][j] |= O.INFO_NONFINITE | O.INFO_TERMINATED
    with pytest.raises(AssertionError), np.errstate(invalid="ignore"):
        B.compare(g, o, m, "f32", GUARD_AUTO)
    g = copy.deepcopy(o)
    g["terminal_obs"][k] = 7.0                                         # unspecified: not compared
    with np.errstate(invalid="ignore"):
        B.compare(g, o, m, "f32", GUARD_AUTO)


def test_compare_gates_an_ended_env_that_is_not_reset_like_one_that_goes_on():
    cfg, _, run = flag_run("quad", 300, "f32", "v2", PLAIN)
    pre, a, o, post, _, _ = run[0]
    m = B.margins(cfg, pre, post)
    k = _pick((o["done"] != 0) & (m["reward"] > 1e-2))
    assert not (o["info"][k] & O.INFO_WAS_RESET) and np.array_equal(o["fstate"][:13, k], post[0][:13, k])
    B.compare(copy.deepcopy(o), o, m, "f32", PLAIN)
    g = copy.deepcopy(o)
    g["fstate"][3, k] += 1e-4 * max(1.0, abs(g["fstate"][3, k]))
    with pytest.raises(AssertionError):
        B.compare(g, o, m, "f32", PLAIN)
    with pytest.raises(AssertionError):                                # ... and the flag word is part of the comparison
        B.compare(copy.deepcopy(o), o, m, "f32", O.FLAG_AUTO_RESET)
