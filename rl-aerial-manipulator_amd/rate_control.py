"""Body-rate actions with an inner rate loop on the rigid vehicles (include/amenv.h amenv_set_rate_control).

The loop runs inside the step / rollout kernels, as a rewrite of the action row in front of the unchanged step: this module only holds and
checks its six numbers and the feed-forward flag.  There is no CPU path."""
import math

from . import _lib as L

MAX_RATE = (5.0, 5.0, 2.5)   # rad/s per unit of action, body x, y, z (the observation scales rates by 5)
GAIN = (25.0, 25.0, 10.0)    # 1/s


def _triple(name, v):
    try:
        v = [x.item() if hasattr(x, "item") else x for x in v]
    except TypeError:
        raise L.AmenvError(f"RateControl: {name} must be three numbers (body x, y, z), got {v!r}") from None
    if len(v) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in v):
        raise L.AmenvError(f"RateControl: {name} must be three numbers (body x, y, z), got {v!r}")
    v = tuple(float(x) for x in v)
    if not all(math.isfinite(x) and x > 0.0 for x in v):
        raise L.AmenvError(f"RateControl: {name} = {v} must be finite and > 0")
    return v


class RateControl:
    """Entries 1..3 of an action row are body-rate commands in units of `max_rate` (rad/s); a proportional rate loop with `gain` (1/s) on
    the vehicle's nominal inertia, plus the gyroscopic feed-forward w x (I w), turns them into the moments the step applies.  The thrust
    entry keeps its meaning.  No integral or derivative term and no state.

    >>> env = GpuWaypointEnv(4096, vehicle="hexa", rate_control=RateControl())
    """

    def __init__(self, max_rate=MAX_RATE, gain=GAIN, gyro_feedforward=True):
        self.max_rate = _triple("max_rate", max_rate)
        self.gain = _triple("gain", gain)
        if not isinstance(gyro_feedforward, (bool, int)):
            raise L.AmenvError(f"RateControl: gyro_feedforward must be a bool, got {gyro_feedforward!r}")
        self.gyro_feedforward = bool(gyro_feedforward)

    def validate(self, dt):
        """The check that needs the control period: gain * dt < 1 on every axis (past that bound the held torque overshoots the command
        within one step).  Returns self."""
        dt = float(dt)
        for k, g in zip("xyz", self.gain):
            if not g * dt < 1.0:
                raise L.AmenvError(f"RateControl: gain {k} = {g} with dt = {dt} gives gain * dt = {g * dt:g}; it must be < 1")
        return self

    def to_c(self):
        c = L.RateControlC()
        for k in range(3):
            c.max_rate[k], c.gain[k] = self.max_rate[k], self.gain[k]
        c.gyro_feedforward, c.reserved = int(self.gyro_feedforward), 0
        return c

    def __repr__(self):
        return f"RateControl(max_rate={self.max_rate}, gain={self.gain}, gyro_feedforward={self.gyro_feedforward})"
