"""Reference side of the rate-control tests (include/amenv.h amenv_set_rate_control): the law restated in numpy, fp64,
in the device function's operation order (csrc/amenv_model.hpp rate_to_moment):

    w_cmd_k = a_k * max_rate_k;   u_k = gain_k * (w_cmd_k - w_k)
    tau_k   = I_k0 u_0 + (I_k1 u_1 + I_k2 u_2)            (the device: fma(I_k0, u_0, fma(I_k1, u_1, I_k2 * u_2)))
    tau    += w x (I w)  with gyro_feedforward             (I w rows as above; cross_k = w_i (Iw)_j - w_j (Iw)_i)
    a'_k    = tau_k * inv_ms

The constants are taken AS THE DEVICE HOLDS THEM: the inertia, max_rate and gain rounded to float32, inv_ms = float32(1 / float32(ms)); what
is compared is then the rounding of the device function's own operations.  Its longest path has N_ROUNDINGS = 8 of them (w_cmd, the
difference, u, the product and the two fmas of the I u row, the sum with the feed-forward, the scaling); the feed-forward's own path has 6
in front of that sum.  Every rounding is relative to a partial result whose magnitude the sum S_k of the absolute values of every term that
enters a'_k bounds, so |a'_k(device) - a'_k(fp64)| <= N_ROUNDINGS * 2^-24 * S_k."""
import numpy as np

N_ROUNDINGS = 8
MAX_RATE = (5.0, 5.0, 2.5)
GAIN = (25.0, 25.0, 10.0)


def device_constants(cfg, max_rate=MAX_RATE, gain=GAIN):
    """(I [3, 3], max_rate [3], gain [3], inv_ms) as fp64 arrays holding the float32 values the kernels are handed; I is the config's NOMINAL inertia."""
    I = np.array(cfg.vehicle.inertia[:9], np.float64).reshape(3, 3).astype(np.float32).astype(np.float64)
    I = np.triu(I) + np.triu(I, 1).T          # the kernels hold the symmetric part's upper triangle (HotParams Ixx .. Izz)
    ms = np.float32(cfg.vehicle.moment_scale)
    return (I, np.asarray(max_rate, np.float32).astype(np.float64), np.asarray(gain, np.float32).astype(np.float64),
            float(np.float32(1.0 / np.float64(ms))))


def moment_actions(actions, w, I, max_rate, gain, inv_ms, gyro_feedforward=True):
    """actions [N, 4], w [N, 3] body rates -> (a' rows [N, 4] fp64 with the thrust column copied, S [N, 3])."""
    a = np.asarray(actions, np.float64)
    w = np.asarray(w, np.float64)
    w_cmd = a[:, 1:4] * max_rate
    u = gain * (w_cmd - w)
    u_abs = np.abs(gain) * (np.abs(w_cmd) + np.abs(w))
    tau = np.zeros_like(u)
    S = np.zeros_like(u)
    for k in range(3):
        tau[:, k] = I[k, 0] * u[:, 0] + (I[k, 1] * u[:, 1] + I[k, 2] * u[:, 2])
        S[:, k] = np.abs(I[k]) @ u_abs.T
    if gyro_feedforward:
        Iw = np.stack([I[k, 0] * w[:, 0] + (I[k, 1] * w[:, 1] + I[k, 2] * w[:, 2]) for k in range(3)], axis=1)
        Iw_abs = np.abs(w) @ np.abs(I).T
        for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            tau[:, k] += w[:, i] * Iw[:, j] - w[:, j] * Iw[:, i]
            S[:, k] += np.abs(w[:, i]) * Iw_abs[:, j] + np.abs(w[:, j]) * Iw_abs[:, i]
    out = a.copy()
    out[:, 1:4] = tau * inv_ms
    return out, S * abs(inv_ms)


def closed_form_rate(w_cmd, gain, dt, n):
    """A held torque about one principal axis from rest, recomputed every step by the P loop (feed-forward zero on a single axis):
    w_n = w_cmd (1 - (1 - gain dt)^n)."""
    return w_cmd * (1.0 - (1.0 - gain * dt) ** n)
