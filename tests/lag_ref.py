"""Reference side of the rotor-lag tests (include/amenv.h amenv_set_rotor_lag): numpy and the UNCHANGED fp64 oracle.

* the filter restated: per control step and rotor, c = sqrt(t_c), a = a_up if c > w else a_down, w' = fma(a, c - w, w), delivered w'^2;
  a = -expm1(-dt / tau) and the episode-start value w0 are formed in fp64 and rounded once to the handle's dtype;
* the commanded thrusts t_c from the oracle's own action scaling (entries 0..3 of the wrench orc_dynamics_step returns);
* the pinned oracle config: the oracle clamps rotor r to [t_min[r], t_max[r]], so a one-env config with t_min[r] = t_max[r] = t_eff[r]
  delivers exactly t_eff whatever the action says.  It composes with dr_ref.oracle_config (that one scales mix and the inertia, not the
  limits): apply dr_ref first, then pin the limits to the UNSCALED w'^2."""
import math

import numpy as np

from oracle import oracle as O
from tests import dr_ref

NP_DTYPE = {"f32": np.float32, "f64": np.float64}


def _np_dtype(dtype):
    return NP_DTYPE.get(dtype, dtype)


def coefficients(dt, tau_up, tau_down, dtype="f64"):
    """(a_up, a_down) of the handle's dtype: -expm1(-dt / tau) in fp64 from the control period, rounded once."""
    t = _np_dtype(dtype)
    return t(-math.expm1(-float(dt) / float(tau_up))), t(-math.expm1(-float(dt) / float(tau_down)))


def _vehicle_arrays(cfg):
    v = cfg.vehicle
    n = int(v.n_rotors)
    alloc = np.array(v.alloc[:4 * n], np.float64).reshape(n, 4)
    return n, alloc, np.array(v.t_min[:n], np.float64), np.array(v.t_max[:n], np.float64)


def w0(cfg, dtype="f64"):
    """[n_rotors] of dtype: sqrt(clamp(alloc[r] . (mass g, 0, 0, 0), t_min[r], t_max[r])) in fp64 with the config's (nominal) mass."""
    n, alloc, tmin, tmax = _vehicle_arrays(cfg)
    t = alloc[:, 0] * (float(cfg.vehicle.mass) * float(cfg.vehicle.g))
    return np.sqrt(np.maximum(np.minimum(t, tmax), tmin)).astype(_np_dtype(dtype))


def commanded(cfg, action):
    """[n_rotors] fp64: the clamped thrust command of one action on the NOMINAL config: u from the oracle's fp32 action scaling."""
    n, alloc, tmin, tmax = _vehicle_arrays(cfg)
    _, wrench = O.dynamics_step(cfg, np.array([0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float64), np.asarray(action, np.float32)[:4])
    u = wrench[:4]
    # the kernels' order: fma(a0, u0, fma(a1, u1, fma(a2, u2, a3 * u3))); fp64 reassociation is far inside the gates
    t = alloc[:, 0] * u[0] + (alloc[:, 1] * u[1] + (alloc[:, 2] * u[2] + alloc[:, 3] * u[3]))
    return np.maximum(np.minimum(t, tmax), tmin)


def filter(w, t_c, a_up, a_down):   # noqa: A001  (the issue's name for it)
    """w' in fp64: one control step of the first-order lag towards c = sqrt(t_c)."""
    w = np.asarray(w, np.float64)
    c = np.sqrt(np.asarray(t_c, np.float64))
    a = np.where(c > w, np.float64(a_up), np.float64(a_down))
    return w + a * (c - w)


def oracle_config(cfg, t_eff, gid=None):
    """A ONE-env copy of the oracle config `cfg` whose rotors deliver exactly t_eff[r]: t_min[r] = t_max[r] = t_eff[r].
    gid: the env's global id (the oracle's reset draws of the copy are keyed by it)."""
    out = dr_ref.copy_config(cfg)
    out.num_envs = 1
    if gid is not None:
        out.env_id_offset = int(gid)
    for r in range(int(out.vehicle.n_rotors)):
        out.vehicle.t_min[r] = float(t_eff[r])
        out.vehicle.t_max[r] = float(t_eff[r])
    return out


class LaggedOracle:
    """The oracle flown with the lag, for closed-loop checks on the CPU.  The limits are per config, so every env is stepped on a pinned
    one-env config of its own: per step and env the filter above, then one oracle step with t_min = t_max = w'^2."""

    def __init__(self, cfg, tau_up, tau_down=None):
        self.cfg = cfg
        self.n = int(cfg.num_envs)
        self.a_up, self.a_down = coefficients(cfg.task.dt, tau_up, tau_up if tau_down is None else tau_down)
        self.w0 = w0(cfg)
        self.w = np.tile(self.w0, (self.n, 1))
        self.env = O.OracleEnv(cfg)
        self._one = [O.OracleEnv(oracle_config(cfg, self.w0 ** 2, gid=int(cfg.env_id_offset) + i)) for i in range(self.n)]

    def reset(self):
        self.w[:] = self.w0
        return self.env.reset()

    def step(self, actions):
        """-> obs [N, OD], done [N], info [N]; auto-reset envs restart their rotors at w0."""
        a = np.ascontiguousarray(actions, np.float32)
        obs = np.zeros((self.n, self.env.obs_dim), np.float32)
        done = np.zeros(self.n, np.uint8)
        info = np.zeros(self.n, np.uint32)
        for i in range(self.n):
            self.w[i] = filter(self.w[i], commanded(self.cfg, a[i]), self.a_up, self.a_down)
            one = self._one[i]
            t = self.w[i] ** 2
            for r in range(len(t)):
                one.cfg.vehicle.t_min[r] = one.cfg.vehicle.t_max[r] = float(t[r])
            one.fstate[:, 0] = self.env.fstate[:, i]
            one.istate[:, 0] = self.env.istate[:, i]
            out = one.step(a[i:i + 1])
            self.env.fstate[:, i] = one.fstate[:, 0]
            self.env.istate[:, i] = one.istate[:, 0]
            obs[i], done[i], info[i] = out["obs"][0], out["done"][0], out["info"][0]
            if info[i] & 128:   # AMENV_INFO_WAS_RESET
                self.w[i] = self.w0
        return obs, done, info
