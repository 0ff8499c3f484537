"""Sensor noise on the rigid vehicles' observations (include/amenv.h amenv_set_sensor_noise).

The noise is drawn and applied inside the step / rollout kernels, on a copy of the state that only the observation reads: this module only
holds and checks the four standard deviations.  There is no CPU path."""
import ctypes
import math

from . import _lib as L

SIGMA_MAX = 1.0   # the C ABI's bound: 0 <= sigma <= 1


def _sigma(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        try:                      # numpy / torch scalars
            v = v.item()
        except (AttributeError, TypeError, ValueError, RuntimeError):
            raise L.AmenvError(f"SensorNoise: {name} must be a number, got {v!r}") from None
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise L.AmenvError(f"SensorNoise: {name} must be a number, got {v!r}")
    v = float(v)
    if not (math.isfinite(v) and 0.0 <= v <= SIGMA_MAX):
        raise L.AmenvError(f"SensorNoise: {name} = {v} must be finite with 0 <= sigma <= {SIGMA_MAX:g}")
    return v


class SensorNoise:
    """Standard deviations of the zero-mean noise on what the policy observes: position (m), velocity (m/s), body rate (rad/s) and
    attitude (rad, a small random rotation).  All 0 = off.  Reward, termination and the state itself stay exact.

    >>> env = GpuWaypointEnv(4096, vehicle="quad", sensor_noise=SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01))
    """

    def __init__(self, position=0.0, velocity=0.0, rate=0.0, attitude=0.0):
        self.position = _sigma("position", position)
        self.velocity = _sigma("velocity", velocity)
        self.rate = _sigma("rate", rate)
        self.attitude = _sigma("attitude", attitude)

    @property
    def sigmas(self):
        return (self.position, self.velocity, self.rate, self.attitude)

    def is_off(self):
        return not any(self.sigmas)

    def to_c(self):
        c = L.SensorNoiseC()
        c.struct_size = ctypes.sizeof(L.SensorNoiseC)
        c.sigma_position, c.sigma_velocity, c.sigma_rate, c.sigma_attitude = self.sigmas
        return c

    def __repr__(self):
        return f"SensorNoise(position={self.position}, velocity={self.velocity}, rate={self.rate}, attitude={self.attitude})"
