"""Reference side of the dynamics-randomisation tests (include/amenv.h amenv_set_randomization).

* a numpy restatement of the factor draw: one Philox block (the oracle's) at block index 0x44520000, eight 16-bit uniforms, fp32
  factor = lo + (hi - lo) * u (a multiply, then an add);
* the per-env oracle config: the UNCHANGED fp64 oracle computes the randomised dynamics when it is given
    inertia' = kI I,  inv_inertia' = inv_inertia / kI,  mix'[0][r] = s_r / km,  mix'[1..3][r] = s_r mix[1..3][r]
  with the nominal mass (action scaling stays nominal): F' / m = sum s_r t_r / (km m) and
  inv_inertia' (M' - w x I' w) = J (M / kI - w x I w)  with M = mix[1..3] (s . t), up to fp64 reassociation."""
import ctypes as C

import numpy as np

from oracle import oracle as O

DR_BLOCK = 0x44520000


def uniforms(seed, gid, episode):
    """The eight 16-bit uniforms of (seed, global env id, episode): u[2k] = low half of word k, u[2k+1] = high half, times 2^-16."""
    w = O.philox(int(seed), int(gid), int(episode) & 0xFFFFFFFF, DR_BLOCK)
    u = np.zeros(8, np.float32)
    for k in range(4):
        u[2 * k] = np.float32(int(w[k]) & 0xFFFF) * np.float32(2.0 ** -16)
        u[2 * k + 1] = np.float32(int(w[k]) >> 16) * np.float32(2.0 ** -16)
    return u


def factor(lo, hi, u):
    """fp32: lo + (hi - lo) * u, a rounded multiply followed by a rounded add."""
    lo, hi, u = np.float32(lo), np.float32(hi), np.float32(u)
    span = np.float32(hi - lo)
    return np.float32(lo + np.float32(span * u))


def factors(seed, gid, episode, n_rotors, mass=(1.0, 1.0), inertia=(1.0, 1.0), thrust=(1.0, 1.0)):
    """[2 + n_rotors] f32: km, kI, s_0.. of one (env, episode)."""
    u = uniforms(seed, gid, episode)
    f = [factor(*mass, u[0]), factor(*inertia, u[1])] + [factor(*thrust, u[2 + r]) for r in range(n_rotors)]
    return np.array(f, np.float32)


def factors_all(seed, gid0, episodes, n_rotors, r):
    """[N, 2 + n_rotors] f32 for envs gid0 .. gid0 + N - 1 at their episode counters; r: a DynamicsRandomization (or None = off)."""
    rng = {} if r is None else dict(mass=r.mass, inertia=r.inertia, thrust=r.thrust)
    return np.stack([factors(seed, gid0 + i, int(ep), n_rotors, **rng) for i, ep in enumerate(np.asarray(episodes))])


def copy_config(cfg):
    out = O.Config()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(O.Config))
    return out


def oracle_config(cfg, f, gid=None):
    """A ONE-env copy of the oracle config `cfg` whose dynamics are those of the factors f = [km, kI, s_0..] (see the module text).
    gid: the env's global id (the oracle's reset draws of the copy are keyed by it)."""
    out = copy_config(cfg)
    out.num_envs = 1
    if gid is not None:
        out.env_id_offset = int(gid)
    v = out.vehicle
    n = v.n_rotors
    km, ki = float(f[0]), float(f[1])
    s = [float(x) for x in f[2:2 + n]]
    for k in range(9):
        v.inertia[k] = v.inertia[k] * ki
        v.inv_inertia[k] = v.inv_inertia[k] / ki
    for r in range(n):
        v.mix[r] = v.mix[r] * s[r] / km              # row 0 is all ones: s_r / km
        for i in range(1, 4):
            v.mix[i * n + r] = v.mix[i * n + r] * s[r]
    return out
