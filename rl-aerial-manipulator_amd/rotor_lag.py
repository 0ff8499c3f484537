"""First-order rotor lag of the rigid vehicles (include/amenv.h amenv_set_rotor_lag).

The filter runs inside the step / rollout kernels, on one state number per env and rotor: this module only holds and checks the two time
constants.  There is no CPU path."""
import ctypes
import math

from . import _lib as L

TAU_MAX = 10.0   # the C ABI's bound: 0 < tau <= 10 s


def _tau(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        try:                      # numpy / torch scalars
            v = v.item()
        except (AttributeError, TypeError, ValueError, RuntimeError):
            raise L.AmenvError(f"RotorLag: {name} must be a number of seconds, got {v!r}") from None
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise L.AmenvError(f"RotorLag: {name} must be a number of seconds, got {v!r}")
    v = float(v)
    if not (math.isfinite(v) and 0.0 < v <= TAU_MAX):
        raise L.AmenvError(f"RotorLag: {name} = {v} must be finite with 0 < tau <= {TAU_MAX:g} (seconds)")
    return v


class RotorLag:
    """Time constants (s) of the rotors' first-order speed response: tau_up while a rotor speeds up, tau_down while it slows down
    (None = tau_up).  The default is the hexacopter model's timeConstantUp = timeConstantDown = 0.015 s, three control steps.

    >>> env = GpuWaypointEnv(4096, vehicle="hexa", rotor_lag=RotorLag(0.015))
    """

    def __init__(self, tau_up=0.015, tau_down=None):
        self.tau_up = _tau("tau_up", tau_up)
        self.tau_down = self.tau_up if tau_down is None else _tau("tau_down", tau_down)

    def coefficients(self, dt):
        """(a_up, a_down) = -expm1(-dt / tau) in fp64 for the control period dt: the share of the gap a rotor closes per control step."""
        return -math.expm1(-float(dt) / self.tau_up), -math.expm1(-float(dt) / self.tau_down)

    def to_c(self):
        c = L.RotorLagC()
        c.struct_size = ctypes.sizeof(L.RotorLagC)
        c.tau_up, c.tau_down = self.tau_up, self.tau_down
        return c

    def __repr__(self):
        return f"RotorLag(tau_up={self.tau_up}, tau_down={self.tau_down})"
