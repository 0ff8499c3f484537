"""Per-episode dynamics randomisation of the rigid vehicles (include/amenv.h amenv_set_randomization).

The factors are drawn inside the step / rollout kernels from (seed, global env id, episode): this module only holds and checks the
ranges.  There is no CPU path."""
import ctypes
import math

import numpy as np

from . import _lib as L

LO_MIN, HI_MAX = 0.25, 4.0   # the C ABI's bounds on every range


def _range(name, v):
    try:
        lo, hi = (float(np.float32(x)) for x in v)   # the kernels see fp32 bounds: check those
    except (TypeError, ValueError):
        raise L.AmenvError(f"DynamicsRandomization: {name} must be a (lo, hi) pair of numbers, got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and LO_MIN <= lo <= hi <= HI_MAX):
        raise L.AmenvError(f"DynamicsRandomization: {name} = ({lo}, {hi}) must be finite with {LO_MIN} <= lo <= hi <= {HI_MAX}")
    return lo, hi


class DynamicsRandomization:
    """Uniform ranges of the per-episode factors: mass (km: the body's mass is km m; actions keep the nominal scaling), inertia (kI: the
    inertia is kI I) and thrust (s_r: rotor r delivers s_r times its clamped command; one draw per rotor).  (1, 1) fixes a factor at 1.

    >>> env = GpuWaypointEnv(4096, randomization=DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.8, 1.2), thrust=(0.95, 1.05)))
    """

    def __init__(self, mass=(1.0, 1.0), inertia=(1.0, 1.0), thrust=(1.0, 1.0)):
        self.mass = _range("mass", mass)
        self.inertia = _range("inertia", inertia)
        self.thrust = _range("thrust", thrust)

    @classmethod
    def around_one(cls, mass=0.0, inertia=0.0, thrust=0.0):
        """Ranges of +-f around 1 (f = 0.2: [0.8, 1.2])."""
        return cls(mass=(1.0 - mass, 1.0 + mass), inertia=(1.0 - inertia, 1.0 + inertia), thrust=(1.0 - thrust, 1.0 + thrust))

    def to_c(self):
        r = L.Randomization()
        r.struct_size = ctypes.sizeof(L.Randomization)
        r.mass_scale[:] = self.mass
        r.inertia_scale[:] = self.inertia
        r.thrust_scale[:] = self.thrust
        return r

    def __repr__(self):
        return f"DynamicsRandomization(mass={self.mass}, inertia={self.inertia}, thrust={self.thrust})"

