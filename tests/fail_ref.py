"""Reference side of the rotor-failure tests (include/amenv.h amenv_set_rotor_failure).

* a numpy restatement of the plan of one (env, episode), operation for operation: one Philox block (the oracle's) at counter word
  0x46410000, four 16-bit halves cut as dr_ref.uniforms cuts them, integer compares and products, and dr_ref.factor's fp32 arithmetic for
  the remaining fraction;
* the multipliers in effect at a step;
* the per-env oracle config: dr_ref.oracle_config on the episode's factors with s_r scaled -- a failed rotor is a scaled mixer column of
  the UNCHANGED fp64 oracle."""
import numpy as np

from oracle import oracle as O
from tests import dr_ref

FAIL_BLOCK = 0x46410000


def halves(seed, gid, episode):
    """v0..v3: low half of word 0, high half of word 0, low half of word 1, high half of word 1."""
    w = O.philox(int(seed), int(gid), int(episode) & 0xFFFFFFFF, FAIL_BLOCK)
    return int(w[0]) & 0xFFFF, int(w[0]) >> 16, int(w[1]) & 0xFFFF, int(w[1]) >> 16


def p16(probability):
    """floor(probability * 65536 + 0.5), in fp64, of the fp32 value the C struct carries"""
    return int(np.floor(np.float64(np.float32(probability)) * 65536.0 + 0.5))


def plan(seed, gid, episode, n_rotors, params):
    """(rotor, onset, f) of one (env, episode); rotor = -1 (and onset = 0): no failure in this episode.  params: a RotorFailure.
    f is the fp32 remaining fraction the draw forms whether or not the episode has a failure."""
    v0, v1, v2, v3 = halves(seed, gid, episode)
    admissible = list(range(n_rotors)) if params.rotors is None else sorted(params.rotors)
    f = dr_ref.factor(params.remaining[0], params.remaining[1], np.float32(v3) * np.float32(2.0 ** -16))
    if not v0 < p16(params.probability):
        return -1, 0, f
    rotor = admissible[(v1 * len(admissible)) >> 16]
    lo, hi = params.onset
    onset = lo + ((v2 * (hi - lo + 1)) >> 16)
    return rotor, onset, f


def plans_all(seed, gid0, episodes, n_rotors, params):
    """(plan [N, 2] int32, f [N] f32) for envs gid0 .. gid0 + N - 1 at their episode counters"""
    rows = [plan(seed, gid0 + i, int(ep), n_rotors, params) for i, ep in enumerate(np.asarray(episodes))]
    return np.array([[r, o] for r, o, _ in rows], np.int32), np.array([f for _, _, f in rows], np.float32)


def effective(pl, step, n_rotors):
    """[n_rotors] f32: the multipliers on s_r in the control step that finds the step field `step`: f on the failed rotor once
    step >= onset, else 1."""
    rotor, onset, f = pl
    out = np.ones(n_rotors, np.float32)
    if rotor >= 0 and int(step) >= onset:
        out[rotor] = np.float32(f)
    return out


def effective_all(plans, f, steps, n_rotors):
    return np.stack([effective((int(p[0]), int(p[1]), x), int(s), n_rotors) for p, x, s in zip(plans, f, np.asarray(steps))])


def oracle_config(base, dr_factors, fail_factors, gid=None, dtype="f64"):
    """dr_ref.oracle_config on [km, kI, s_0 * x_0, ..]: the thrust factors as the kernel of `dtype` holds them, one rounded multiply in its
    type (fp32: of the two float32 values; fp64: of their exact fp64 images)."""
    f = np.array(dr_factors, np.float64)
    n = len(fail_factors)
    if dtype == "f64":
        f[2:2 + n] = np.asarray(dr_factors[2:2 + n], np.float64) * np.asarray(fail_factors, np.float64)
    else:
        f[2:2 + n] = (np.asarray(dr_factors[2:2 + n], np.float32) * np.asarray(fail_factors, np.float32)).astype(np.float64)
    return dr_ref.oracle_config(base, f, gid=gid)
