"""Per-episode actuation latency on the rigid vehicles (include/amenv.h amenv_set_action_delay).

The delay is drawn and the action history is kept inside the step / rollout kernels: this module only holds and checks the range of
control steps.  There is no CPU path."""
import ctypes

from . import _lib as L

MAX_ACTION_DELAY = L.MAX_ACTION_DELAY   # the C ABI's bound: 8 control steps, 40 ms at 200 Hz


def _steps(name, v):
    if isinstance(v, bool) or not isinstance(v, int):
        try:                      # numpy / torch integer scalars
            w = v.item()
        except (AttributeError, TypeError, ValueError, RuntimeError):
            raise L.AmenvError(f"ActionDelay: {name} must be an integer number of control steps, got {v!r}") from None
        if isinstance(w, bool) or not isinstance(w, int):
            raise L.AmenvError(f"ActionDelay: {name} must be an integer number of control steps, got {v!r}")
        v = w
    return int(v)


class ActionDelay:
    """Each env applies the action it was given `d` control steps ago; `d` is drawn per episode, uniformly from min_steps..max_steps
    (max_steps defaults to min_steps: a fixed delay).  Until an episode is d steps old the vehicle gets the hover action (1, 0, 0, 0).
    Neither d nor the pending actions are observed.

    >>> env = GpuWaypointEnv(4096, vehicle="quad", action_delay=ActionDelay(0, 4))
    """

    def __init__(self, min_steps, max_steps=None):
        self.min_steps = _steps("min_steps", min_steps)
        self.max_steps = self.min_steps if max_steps is None else _steps("max_steps", max_steps)
        if not 0 <= self.min_steps <= self.max_steps <= MAX_ACTION_DELAY:
            raise L.AmenvError(f"ActionDelay: need 0 <= min_steps <= max_steps <= {MAX_ACTION_DELAY}, got ({self.min_steps}, {self.max_steps})")

    def _as_c(self):
        c = L.ActionDelayC()
        c.struct_size = ctypes.sizeof(L.ActionDelayC)
        c.min_steps, c.max_steps = self.min_steps, self.max_steps
        return c

    def __repr__(self):
        return f"ActionDelay({self.min_steps}, {self.max_steps})"
