"""Per-episode rotor failure on the rigid vehicles (include/amenv.h amenv_set_rotor_failure).

The plan is drawn and applied inside the step / rollout kernels, as one more factor on a rotor's thrust factor: this module only holds and
checks the parameters.  There is no CPU path."""
import math

from . import _lib as L

MAX_ONSET = 65535


def _number(name, x):
    x = x.item() if hasattr(x, "item") else x
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise L.AmenvError(f"RotorFailure: {name} must be a number, got {x!r}")
    return x


def _pair(name, v):
    try:
        v = list(v)
    except TypeError:
        raise L.AmenvError(f"RotorFailure: {name} must be a (lo, hi) pair, got {v!r}") from None
    if len(v) != 2:
        raise L.AmenvError(f"RotorFailure: {name} must be a (lo, hi) pair, got {v!r}")
    return _number(name, v[0]), _number(name, v[1])


class RotorFailure:
    """With `probability` an episode has one rotor failure: one of `rotors` (None = any), drawn per episode, delivers from control step
    `onset` (inclusive integer range, drawn per episode) on only the fraction `remaining` (range, drawn per episode; 0 = a dead rotor) of
    its thrust.  A pure function of (seed, env id, episode, these parameters); the failure is not observed.

    >>> env = GpuWaypointEnv(4096, vehicle="hexa", rotor_failure=RotorFailure(probability=0.3, onset=(50, 400), remaining=(0.0, 0.5)))
    """

    def __init__(self, probability=1.0, onset=(0, 0), remaining=(0.0, 0.0), rotors=None):
        p = float(_number("probability", probability))
        if not (math.isfinite(p) and 0.0 <= p <= 1.0):
            raise L.AmenvError(f"RotorFailure: probability = {p} must be finite, 0..1")
        lo, hi = _pair("onset", onset)
        if not (isinstance(lo, int) and isinstance(hi, int)):
            raise L.AmenvError(f"RotorFailure: onset = {(lo, hi)} must be a range of whole control steps")
        if not 0 <= lo <= hi <= MAX_ONSET:
            raise L.AmenvError(f"RotorFailure: onset = {(lo, hi)} must satisfy 0 <= lo <= hi <= {MAX_ONSET}")
        rlo, rhi = (float(x) for x in _pair("remaining", remaining))
        if not (math.isfinite(rlo) and math.isfinite(rhi) and 0.0 <= rlo <= rhi <= 1.0):
            raise L.AmenvError(f"RotorFailure: remaining = {(rlo, rhi)} must be finite with 0 <= lo <= hi <= 1")
        if rotors is not None:
            try:
                rotors = [_number("rotors", r) for r in rotors]
            except TypeError:
                raise L.AmenvError(f"RotorFailure: rotors must be None or rotor indices, got {rotors!r}") from None
            if len(rotors) == 0 or any(not isinstance(r, int) or not 0 <= r < L.MAX_ROTORS for r in rotors) or len(set(rotors)) != len(rotors):
                raise L.AmenvError(f"RotorFailure: rotors = {rotors} must be a non-empty set of distinct rotor indices")
            rotors = tuple(sorted(rotors))
        self.probability, self.onset, self.remaining, self.rotors = p, (lo, hi), (rlo, rhi), rotors

    def validate(self, n_rotors):
        """The check that needs the vehicle: every index of `rotors` is one of its rotors.  Returns self."""
        if self.rotors is not None and self.rotors[-1] >= n_rotors:
            raise L.AmenvError(f"RotorFailure: rotors = {self.rotors} on a vehicle with {n_rotors} rotors")
        return self

    @property
    def rotor_mask(self):
        """bit r: rotor r may fail; 0 = all"""
        return 0 if self.rotors is None else sum(1 << r for r in self.rotors)

    def to_c(self):
        c = L.RotorFailureC()
        c.struct_size = L.C.sizeof(L.RotorFailureC)
        c.probability = self.probability
        c.onset_min, c.onset_max = self.onset
        c.remaining_min, c.remaining_max = self.remaining
        c.rotor_mask = self.rotor_mask
        return c

    def __repr__(self):
        return f"RotorFailure(probability={self.probability}, onset={self.onset}, remaining={self.remaining}, rotors={self.rotors})"
