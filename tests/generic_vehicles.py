"""Fully general vehicles and task constants for the tests that pin the kernels to the oracle (tests/test_generic_vehicles_cpu.py,
tests/test_gpu_generic_vehicles.py): every entry of amenv_vehicle that the default parameter sets leave zero, equal over the rotors or
symmetric is non-zero, different and asymmetric here, so that a term dropped, transposed or read from the wrong index changes the step.
numpy, ctypes and the oracle only: no GPU, no torch.

The builders overwrite cfg.vehicle / cfg.task in place and take an oracle.Config or the package's Config (same layout).  Every number is a
literal below; DESIGN.md 4w says why each is what it is, tests/test_generic_vehicles_cpu.py asserts the properties, and `mutations` is the
table of single reverts each of which must change one oracle step by far more than the gates."""
import ctypes as C

import numpy as np

from oracle import oracle as O

G = 9.6                                   # not 9.81
DT, COUNTER_LIMIT, MAX_EPISODE_STEPS = 0.004, 7, 37
DEFAULT_DT, DEFAULT_G = 1.0 / 200.0, 9.81
DEFAULT_MOMENT_SCALE = {4: 0.1, 6: 1.0}
MOMENT_SCALE = {4: 0.13, 6: 0.8}
# the axes the principal frames of the six inertia tensors are turned about (quad, hexa, arm base, links 1..3): no axis near a coordinate
# axis or plane, so that all three products of inertia are of one size
TILT_AXIS = [(0.5, -0.6, 0.62), (-0.55, 0.47, 0.69), (0.61, 0.58, -0.54), (0.48, -0.66, -0.58), (-0.63, -0.5, 0.59), (0.57, 0.52, 0.63)]
AXES = {"zxx": (0, 0, 1, 1, 0, 0, 1, 0, 0), "yzx": (0, 1, 0, 0, 0, 1, 1, 0, 0),
        # three unit axes without a zero component (0.36^2 + 0.48^2 + 0.8^2 = 0.6^2 + 0.64^2 + 0.48^2 = 1)
        "skew": (0.36, -0.48, 0.8, 0.6, 0.64, -0.48, -0.48, 0.6, 0.64)}


def _rotation(axis, angle):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def full_inertia(principal, axis, angle):
    """A full symmetric positive-definite tensor: the principal moments turned by `angle` about `axis`."""
    R = _rotation(axis, angle)
    I = R @ np.diag(principal) @ R.T
    return 0.5 * (I + I.T)


def _put(arr, values):
    v = np.asarray(values, np.float64).reshape(-1)
    for j in range(len(v)):
        arr[j] = float(v[j])


def _set_inertia(v, I):
    _put(v.inertia, I); _put(v.inv_inertia, np.linalg.inv(I))


def _rigid(cfg, n_rotors, mass, I, x, y, spin_mc, t_min, t_max):
    v = cfg.vehicle
    C.memset(C.byref(v), 0, C.sizeof(v))
    v.n_rotors, v.n_joints, v.mass, v.g, v.moment_scale = n_rotors, 0, mass, G, MOMENT_SCALE[n_rotors]
    _set_inertia(v, I)
    # total thrust the plain sum (row 0), roll moment y_r, pitch moment -x_r, yaw moment spin_r * (the rotor's own moment constant)
    mix = np.stack([np.ones(n_rotors), np.asarray(y, float), -np.asarray(x, float), np.asarray(spin_mc, float)])
    _put(v.mix, mix); _put(v.alloc, np.linalg.pinv(mix))
    _put(v.t_min, t_min); _put(v.t_max, t_max)
    return cfg


def generic_quad(cfg):
    """4 rotors: the reference quadrotor's size, nothing zero, equal or symmetric."""
    I = full_inertia([2.1e-4, 2.9e-4, 4.3e-4], TILT_AXIS[0], 0.6)
    return _rigid(cfg, 4, 0.21, I, x=[0.091, 0.004, -0.083, -0.007], y=[0.005, 0.089, -0.006, -0.081],
                  spin_mc=[0.0262, -0.0231, 0.0249, -0.0274], t_min=[0.020, 0.035, 0.050, 0.027], t_max=[0.93, 0.81, 1.02, 0.88])


HEXA_X = [-0.249, 0.262, -0.258, 0.247, 0.011, -0.013]
HEXA_Y = [0.151, -0.143, -0.156, 0.139, 0.301, -0.288]
HEXA_SPIN_MC = [0.0171, -0.0159, -0.0182, 0.0164, -0.0176, 0.0155]
HEXA_T_MIN = [2.6, 3.4, 2.2, 3.0, 3.7, 2.4]
HEXA_T_MAX = [9.1, 8.3, 9.8, 8.7, 10.4, 7.9]


def generic_hexa(cfg):
    """6 rotors: the hexacopter's size; per-rotor thrust ranges tight enough that both clamps act on many envs of a random action batch."""
    I = full_inertia([3.9e-2, 5.1e-2, 8.2e-2], TILT_AXIS[1], 0.5)
    return _rigid(cfg, 6, 2.93, I, HEXA_X, HEXA_Y, HEXA_SPIN_MC, HEXA_T_MIN, HEXA_T_MAX)


BASE_MASS = 2.95
LINK_MASS = [0.19, 0.13, 0.31]
JOINT_ORIGIN = [0.0131, -0.0142, -0.0985, 0.0087, 0.0163, -0.0114, -0.0093, 0.0121, -0.1010]
LINK_COM = [0.0112, -0.0094, -0.0231, 0.0073, -0.0088, -0.0490, 0.0066, -0.0061, -0.0790]
TOOL_OFFSET = [-0.0115, 0.0132, -0.1190]
JOINT_LIMIT = [-2.6, 3.0, -1.2, 1.7, -1.6, 1.1]
JOINT_KP, JOINT_KD, JOINT_ACC_MAX = 81.0, 17.0, 11.0
# principal moments of the links; link 1's are far above the SDF link's (2e-5) so that its products of inertia move the base by more than
# the gates within one step (tests/test_generic_vehicles_cpu.py, the detection table)
LINK_PRINCIPAL = [[6.0e-3, 9.0e-3, 1.4e-2], [3.0e-3, 5.2e-3, 8.0e-3], [2.4e-3, 4.6e-3, 7.0e-3]]
LINK_TILT = [0.7, 0.6, 0.8]


def generic_arm(cfg, n_joints=3, axes="zxx"):
    """The 6-rotor vehicle of generic_hexa with an arm of n_joints links: axes "zxx" (the fast path), "yzx" or "skew" (the general body)."""
    assert n_joints in (1, 2, 3) and axes in AXES, (n_joints, axes)
    base = full_inertia([4.1e-2, 4.9e-2, 7.9e-2], TILT_AXIS[2], 0.5)
    links = [full_inertia(LINK_PRINCIPAL[k], TILT_AXIS[3 + k], LINK_TILT[k]) for k in range(3)]
    _rigid(cfg, 6, BASE_MASS + sum(LINK_MASS[:n_joints]), base, HEXA_X, HEXA_Y, HEXA_SPIN_MC, HEXA_T_MIN, HEXA_T_MAX)
    v = cfg.vehicle
    v.n_joints = n_joints
    _put(v.joint_origin, JOINT_ORIGIN); _put(v.joint_axis, AXES[axes]); _put(v.link_mass, LINK_MASS); _put(v.link_com, LINK_COM)
    _put(v.link_inertia, np.concatenate([I.reshape(-1) for I in links]))
    v.joint_kp, v.joint_kd, v.joint_acc_max, v.joint_reserved = JOINT_KP, JOINT_KD, JOINT_ACC_MAX, 0.0
    _put(v.joint_limit, JOINT_LIMIT); _put(v.tool_offset, TOOL_OFFSET)
    return cfg


def generic_task(cfg):
    """A step, a hold and an episode of other lengths than the reference's: a hold ends inside six steps."""
    cfg.task.dt, cfg.task.counter_limit, cfg.task.max_episode_steps = DT, COUNTER_LIMIT, MAX_EPISODE_STEPS
    return cfg


def build(cfg, vehicle):
    """Overwrite cfg with the generic vehicle named `vehicle` ("gen_quad", "gen_hexa", "gen_arm", "gen_arm_2j", "gen_arm_base",
    "gen_arm_yzx", "gen_arm_skew") and the generic task constants; ee_task: the base on "gen_arm_base" and the rigid vehicles, else the tool."""
    assert vehicle in VEHICLES, vehicle
    if vehicle == "gen_quad":
        generic_quad(cfg)
    elif vehicle == "gen_hexa":
        generic_hexa(cfg)
    else:
        generic_arm(cfg, n_joints=2 if vehicle == "gen_arm_2j" else 3, axes=vehicle[8:] if vehicle[8:] in AXES else "zxx")
    cfg.task.ee_task = O.EE_TASK_TOOL if cfg.vehicle.n_joints and vehicle != "gen_arm_base" else O.EE_TASK_BASE
    return generic_task(cfg)


VEHICLES = ("gen_quad", "gen_hexa", "gen_arm", "gen_arm_2j", "gen_arm_base", "gen_arm_yzx", "gen_arm_skew")


def copy_of(cfg):
    return type(cfg).from_buffer_copy(cfg)


def round_to_f32(cfg):
    """A copy of cfg with every floating-point vehicle parameter rounded to fp32, as an fp32 kernel holds it."""
    c = copy_of(cfg)
    for name, ctype in type(c.vehicle)._fields_:
        x = getattr(c.vehicle, name)
        if ctype is C.c_double:
            setattr(c.vehicle, name, float(np.float32(x)))
        elif ctype not in (C.c_int32,):
            for j in range(len(x)):
                x[j] = float(np.float32(x[j]))
    return c


# ---- the detection table: single reverts of a generic config -----------------------------------------------------------------------------------
def _inertia_mut(f):
    def mut(cfg):
        v = cfg.vehicle
        I = f(np.array(v.inertia[:9]).reshape(3, 3).copy())
        _set_inertia(v, I)
    return mut


def _zero_off(I):
    return np.diag(np.diag(I))


def _swap_xy_xz(I):
    I[0, 1], I[0, 2] = I[0, 2], I[0, 1]
    I[1, 0], I[2, 0] = I[0, 1], I[0, 2]
    return I


def _swap(name, i, j):
    def mut(cfg):
        a = getattr(cfg.vehicle, name)
        a[i], a[j] = a[j], a[i]
    return mut


def _zero(name, idx):
    def mut(cfg):
        a = getattr(cfg.vehicle, name)
        for j in idx:
            a[j] = 0.0
    return mut


def _link_zero_off(k):
    def mut(cfg):
        a = cfg.vehicle.link_inertia
        for j in (1, 2, 3, 5, 6, 7):
            a[9 * k + j] = 0.0
    return mut


def _mid_zero(k):
    def mut(cfg):
        a = cfg.vehicle.joint_limit
        h = 0.5 * (a[2 * k + 1] - a[2 * k])
        a[2 * k], a[2 * k + 1] = -h, h
    return mut


def _scalar(where, name, value):
    def mut(cfg):
        setattr(getattr(cfg, where), name, value)
    return mut


def mutations(cfg):
    """[(label, f)]: f(cfg) reverts one parameter group of the generic config `cfg` to its default, or swaps two of its entries, in place."""
    nr, nj = cfg.vehicle.n_rotors, cfg.vehicle.n_joints
    m = [("base inertia off-diagonals zeroed", _inertia_mut(_zero_off)), ("Ixy <-> Ixz", _inertia_mut(_swap_xy_xz)),
         ("t_max of rotors 0, 1 swapped", _swap("t_max", 0, 1)), ("t_min of rotors 0, 1 swapped", _swap("t_min", 0, 1)),
         ("t_max of the last two rotors swapped", _swap("t_max", nr - 2, nr - 1)), ("t_min of the last two rotors swapped", _swap("t_min", nr - 2, nr - 1))]
    for row in (1, 2, 3):
        m.append((f"mix row {row}: rotors 0, 1 swapped", _swap("mix", row * nr, row * nr + 1)))
    alloc = np.array(cfg.vehicle.alloc[:4 * nr]).reshape(nr, 4)
    for col in (0, 1, 2, 3):       # the two rotors whose entries differ most: column 0 (the hover shares) is nearly flat
        lo, hi = int(np.argmin(alloc[:, col])), int(np.argmax(alloc[:, col]))
        m.append((f"alloc column {col}: rotors {lo}, {hi} swapped", _swap("alloc", lo * 4 + col, hi * 4 + col)))
    m += [("g back to 9.81", _scalar("vehicle", "g", DEFAULT_G)), ("moment_scale back to its default", _scalar("vehicle", "moment_scale", DEFAULT_MOMENT_SCALE[nr])),
          ("dt back to 1/200", _scalar("task", "dt", DEFAULT_DT))]
    for k in range(nj):
        m += [(f"link {k + 1} CoM zeroed", _zero("link_com", range(3 * k, 3 * k + 3))), (f"link {k + 1} inertia off-diagonals zeroed", _link_zero_off(k)),
              (f"joint {k + 1} mid zeroed", _mid_zero(k))]
    if nj:
        # the entries of the default joint origins that are zero: joint 2's x and z, joint 3's x and y
        for j in [j for j in (3, 5, 6, 7) if j < 3 * nj]:
            m.append((f"joint_origin[{j}] back to zero", _zero("joint_origin", [j])))
        m.append(("tool_offset[0] zeroed", _zero("tool_offset", [0])))
    return m
