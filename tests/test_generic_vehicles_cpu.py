"""tests/generic_vehicles.py on the oracle alone: what tests/test_gpu_generic_vehicles.py relies on, checked where no GPU is needed.

  1. The parameter sets are what they claim: nothing zero, equal over the rotors or symmetric that the defaults leave so.
  2. The rigid oracle on a full inertia tensor: torque-free, the world angular momentum and the rotational energy hold to the order of the
     integrator (the arm's invariants: tests/test_arm_cpu.py, parametrised over the same vehicles).
  3. Detection: every single revert of `generic_vehicles.mutations` moves one teacher-forced oracle step from the sweep's blob by at least
     1e-3 of a gated output on some env (100 times the fp32 state gate) and by at least 1e-4 on 8 envs or more: a kernel that ignored the
     group, or read its neighbour, cannot pass the GPU comparison.
  4. Conditioning: rounding every vehicle parameter to fp32 moves the same step by at most 1e-6, a tenth of the fp32 gate, so the gates
     of tests/state_blob.py need not move.
(Branch coverage and the flip cap on these vehicles: tests/test_state_blob_cpu.py, GENERIC_STATES.)"""
import itertools

import numpy as np
import pytest

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from tests import generic_vehicles as GV
from tests import state_blob as B
from tests.test_arm_cpu import rot_q
from tests.test_state_blob_cpu import ACTION_SEED, start_state

SIX = (0, 1, 2, 4, 5, 8)          # the distinct entries of a symmetric 3 x 3, row-major


def _cfg(vehicle):
    return GV.build(O.reference_quad_config(1), vehicle)


def _default(vehicle):
    return amd._lib.default_config({"gen_quad": "quad", "gen_hexa": "hexa"}.get(vehicle, "hexa_arm"), 1)


def _distinct(x, rel=1e-3):
    """Pairwise different in magnitude, by more than rel of the larger."""
    x = np.abs(np.asarray(x, float))
    return all(abs(a - b) > rel * max(a, b) for a, b in itertools.combinations(x, 2))


def _assert_full_tensor(I, what):
    six = I.reshape(-1)[list(SIX)]
    assert (six != 0).all() and _distinct(six), (what, six)
    assert np.array_equal(I, I.T) and np.linalg.eigvalsh(I).min() > 0, what


@pytest.mark.parametrize("vehicle", GV.VEHICLES)
def test_generic_parameters_are_general(vehicle):
    cfg, dflt = _cfg(vehicle), _default(vehicle)
    v, d = cfg.vehicle, dflt.vehicle
    nr, nj = v.n_rotors, v.n_joints
    assert nr == d.n_rotors and nj == (2 if vehicle == "gen_arm_2j" else d.n_joints)
    # ---- inertia
    I, J = np.array(v.inertia[:9]).reshape(3, 3), np.array(v.inv_inertia[:9]).reshape(3, 3)
    _assert_full_tensor(I, "inertia")
    assert np.abs(I @ J - np.eye(3)).max() < 1e-13
    # ---- mixer
    mix, alloc = np.array(v.mix[:4 * nr]).reshape(4, nr), np.array(v.alloc[:4 * nr]).reshape(nr, 4)
    assert (mix[0] == 1.0).all()
    for row in mix[1:]:
        assert (row != 0).all() and len(set(row)) == nr and _distinct(row), row
    assert np.abs(alloc - np.linalg.pinv(mix)).max() < 1e-13 and np.abs(mix @ alloc - np.eye(4)).max() < 1e-13
    # ---- rotor limits
    t_min, t_max = np.array(v.t_min[:nr]), np.array(v.t_max[:nr])
    hover = alloc[:, 0] * v.mass * v.g
    assert (t_min > 0).all() and _distinct(t_min) and _distinct(t_max) and (t_min < hover).all() and (hover < t_max).all(), (t_min, hover, t_max)
    # ---- scalars
    assert v.mass != d.mass and v.g != 9.81 and v.g != d.g and v.moment_scale not in (0.1, 1.0, d.moment_scale)
    # ---- task
    assert (cfg.task.dt, cfg.task.counter_limit, cfg.task.max_episode_steps) == (0.004, 7, 37)
    if not nj:
        return
    # ---- arm
    jo, lc, tool = np.array(v.joint_origin[:9]), np.array(v.link_com[:9]), np.array(v.tool_offset[:3])
    assert (jo != 0).all() and (lc != 0).all() and (tool != 0).all()
    for k in range(3):
        _assert_full_tensor(np.array(v.link_inertia[9 * k:9 * k + 9]).reshape(3, 3), f"link {k + 1}")
        lo, hi = v.joint_limit[2 * k], v.joint_limit[2 * k + 1]
        assert lo < 0 < hi and abs(lo + hi) > 0.1, (lo, hi)                       # mid != 0
        assert v.link_mass[k] != d.link_mass[k] and v.link_mass[k] > 0
    assert abs(v.mass - (GV.BASE_MASS + sum(v.link_mass[:nj]))) < 1e-15
    assert v.joint_kp != d.joint_kp and v.joint_kd != d.joint_kd and v.joint_acc_max != d.joint_acc_max
    axes = np.array(v.joint_axis[:9]).reshape(3, 3)
    assert np.abs(np.linalg.norm(axes, axis=1) - 1).max() < 1e-15
    name = vehicle[8:] if vehicle[8:] in GV.AXES else "zxx"
    assert np.array_equal(axes.reshape(-1), np.array(GV.AXES[name], float))
    assert name != "skew" or (axes != 0).all()
    assert name != "zxx" or np.array_equal(axes.reshape(-1), np.array(d.joint_axis[:9]))      # the kernels' fast path


def test_the_builders_take_both_config_types():
    a, b = O.reference_quad_config(1), amd._lib.default_config("hexa_arm", 1)
    GV.generic_arm(a, axes="skew"); GV.generic_arm(b, axes="skew")
    GV.generic_task(a); GV.generic_task(b)
    assert bytes(a.vehicle) == bytes(b.vehicle) and (a.task.dt, a.task.counter_limit, a.task.max_episode_steps) == (b.task.dt, b.task.counter_limit, b.task.max_episode_steps)


# ---- the rigid oracle on a full inertia tensor ------------------------------------------------------------------------------------------------
def _rigid_drift(cfg, steps):
    v = cfg.vehicle
    I = np.array(v.inertia[:9]).reshape(3, 3)
    rng = np.random.RandomState(5)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    s = np.concatenate([[0.3, -0.2, 1.5], [0.4, -0.1, 0.2], q, [2.5, -1.8, 3.1]])
    a = np.array([1.0, 0, 0, 0], np.float32)                       # collective thrust only: hover lies inside every rotor's range

    def invariants(s):
        w = s[10:13]
        return rot_q(s[6:10]).T @ (I @ w), 0.5 * w @ I @ w         # body -> world is rot_q(q).T

    L0, E0 = invariants(s)
    worst = 0.0
    for t in range(steps):
        s, w = O.dynamics_step(cfg, s, a)
        assert np.abs(w[5:8]).max() < 1e-15, w                     # torque-free: the post-mixer moments
        L, E = invariants(s)
        worst = max(worst, np.abs(L - L0).max() / np.abs(L0).max(), abs(E - E0) / E0)
    return worst


@pytest.mark.parametrize("vehicle", ["gen_quad", "gen_hexa"])
def test_torque_free_rigid_body_with_a_full_inertia_conserves_to_the_integrators_order(vehicle):
    cfg = _cfg(vehicle)
    drift = _rigid_drift(cfg, 400)
    cfg.task.dt = cfg.task.dt / 2
    half = _rigid_drift(cfg, 800)
    print(f"{vehicle}: drift {drift:.2e}, at dt/2 {half:.2e}, ratio {drift / half:.2f}")
    assert drift > 0 and 12.0 < drift / half < 20.0, (drift, half)


# ---- detection and conditioning, on the sweep's own blob -----------------------------------------------------------------------------------------
def _step(cfg, vehicle, dtype="f32"):
    _, fs, is_ = start_state(vehicle, 300, dtype)
    a = B.actions(cfg, fs, np.random.RandomState(ACTION_SEED))
    return B.oracle_step(cfg, (fs, is_), a)[0]


def _per_env_change(o, o2):
    """Largest relative change of a gated output, per env: float state, reward, observation row, terminal row, ep_return."""
    e = B.rel_err(o["fstate"], o2["fstate"]).max(axis=0)
    e = np.maximum(e, B.rel_err(o["reward"], o2["reward"]))
    e = np.maximum(e, B.rel_err(o["obs"], o2["obs"]).max(axis=1))
    e = np.maximum(e, np.nan_to_num(B.rel_err(o["terminal_obs"], o2["terminal_obs"])).max(axis=1))
    return np.maximum(e, np.nan_to_num(B.rel_err(o["ep_return"], o2["ep_return"])))


def _table():
    return [(v, label) for v in GV.VEHICLES for label, _ in GV.mutations(_cfg(v))]


@pytest.mark.parametrize("vehicle,label", _table(), ids=[f"{v}-{l}".replace(" ", "_") for v, l in _table()])
def test_every_single_revert_moves_the_step_far_beyond_the_gates(vehicle, label):
    cfg, _, _ = start_state(vehicle, 300, "f32")
    mutated = GV.copy_of(cfg)
    dict(GV.mutations(cfg))[label](mutated)
    assert bytes(mutated) != bytes(cfg)
    e = _per_env_change(_step(cfg, vehicle), _step(mutated, vehicle))
    print(f"{vehicle}: {label}: largest change {e.max():.2e}, envs at 1e-4 or more: {int((e >= 1e-4).sum())}")
    assert e.max() >= 1e-3 and (e >= 1e-4).sum() >= 8, (e.max(), int((e >= 1e-4).sum()))


def test_the_table_holds_every_group_the_defaults_hide():
    labels = {v: [label for label, _ in GV.mutations(_cfg(v))] for v in GV.VEHICLES}
    assert len(labels["gen_quad"]) == len(labels["gen_hexa"]) == 16
    assert len(labels["gen_arm"]) == 16 + 9 + 4 + 1 and len(labels["gen_arm_2j"]) == 16 + 6 + 2 + 1


@pytest.mark.parametrize("vehicle", GV.VEHICLES)
def test_fp32_parameters_move_the_step_by_a_tenth_of_the_gate_at_most(vehicle):
    cfg, _, _ = start_state(vehicle, 300, "f32")
    o, o2 = _step(cfg, vehicle), _step(GV.round_to_f32(cfg), vehicle)
    same = (o["info"] == o2["info"]) & (o["done"] == 0)
    assert same.sum() > 200
    e = B.rel_err(o["fstate"], o2["fstate"])[:, same].max()
    print(f"{vehicle}: parameters rounded to fp32 move the state by {e:.2e}")
    assert e <= 1e-6, e
