"""Reference side of the sensor-noise tests (include/amenv.h amenv_set_sensor_noise).

* a numpy restatement of the samples: three Philox blocks (the oracle's) at counter word 0x4E000000 | ((step & 0x3FFFFF) << 2) | b; word k
  of block b is sample 4 b + k = (float32(sum of the word's four bytes) - 510) * float32(21845^-1/2): integer arithmetic, one exact fp32
  subtraction and one fp32 multiply, so the kernels' samples are reproduced bit for bit;
* expected_obs: the UNCHANGED fp64 oracle's observe() on a copy of the true state whose rows 0..12 are perturbed in fp64 with those samples,
  in the kernels' order: p, v, w += sigma n; d = sigma_a / 2 * n, q~ = q (x) (1, d) (Hamilton, scalar first), renormalised."""
import numpy as np

from oracle import oracle as O

NOISE_TAG = 0x4E000000
SCALE = np.float32(21845.0 ** -0.5)      # 0.006765875: fp32 nearest to 21845^-1/2
BOUND = 510.0 * float(SCALE)             # |n| <= 3.4506


def samples(seed, gid, episode, step):
    """[12] f32: the unit samples of (seed, global env id, episode, step)."""
    n = np.zeros(12, np.float32)
    for b in range(3):
        w = O.philox(int(seed), int(gid), int(episode) & 0xFFFFFFFF, NOISE_TAG | ((int(step) & 0x3FFFFF) << 2) | b)
        for k in range(4):
            x = int(w[k])
            s = (x & 0xFF) + ((x >> 8) & 0xFF) + ((x >> 16) & 0xFF) + (x >> 24)
            n[4 * b + k] = np.float32(np.float32(s) - np.float32(510.0)) * SCALE
    return n


def samples_all(seed, gid0, episodes, steps):
    """[N, 12] f32 for envs gid0 .. gid0 + N - 1 at their (episode, step) counters."""
    return np.stack([samples(seed, gid0 + i, int(ep), int(st)) for i, (ep, st) in enumerate(zip(np.asarray(episodes), np.asarray(steps)))])


def perturb(fstate, n, sigmas):
    """A copy of fstate [NF, N] (fp64) whose rows 0..12 carry the noise of the samples n [N, 12]; sigmas = (position, velocity, rate, attitude)."""
    f = np.array(fstate, np.float64, copy=True)
    n = np.asarray(n, np.float64)
    sp, sv, sw, sa = (float(np.float32(s)) for s in sigmas)
    f[0:3] += sp * n[:, 0:3].T
    f[3:6] += sv * n[:, 3:6].T
    f[10:13] += sw * n[:, 6:9].T
    dx, dy, dz = (0.5 * sa * n[:, 9 + k] for k in range(3))
    qw, qx, qy, qz = f[6], f[7], f[8], f[9]
    tw = qw - qx * dx - qy * dy - qz * dz
    tx = qx + qw * dx + qy * dz - qz * dy
    ty = qy + qw * dy + qz * dx - qx * dz
    tz = qz + qw * dz + qx * dy - qy * dx
    rn = 1.0 / np.sqrt(tw * tw + tx * tx + ty * ty + tz * tz)
    f[6], f[7], f[8], f[9] = tw * rn, tx * rn, ty * rn, tz * rn
    return f


def expected_obs(oracle_cfg, fstate, istate, sigmas, seed, gid0):
    """[N, obs_dim] f32: what a noisy handle observes in the true state (fstate [NF, N], istate [4, N]): the oracle's observe() on the
    perturbed copy, the samples keyed by every env's own (episode, step) fields."""
    fstate = np.asarray(fstate, np.float64)
    istate = np.ascontiguousarray(istate, np.int32)
    n = fstate.shape[1]
    cfg = O.Config.from_buffer_copy(oracle_cfg)
    cfg.num_envs = n
    env = O.OracleEnv(cfg)
    assert env.fstate.shape == fstate.shape, (env.fstate.shape, fstate.shape)
    env.istate[:] = istate
    if any(float(s) != 0.0 for s in sigmas):
        env.fstate[:] = perturb(fstate, samples_all(seed, gid0, istate[O.I_EPISODE], istate[O.I_STEP]), sigmas)
    else:
        env.fstate[:] = fstate
    return env.observe()
