"""Action history in the rigid vehicles' observation rows (include/amenv.h amenv_set_action_history).

The rows are kept and appended inside the step / rollout kernels (they are the action delay's side buffer): this module only holds and
checks the number of rows.  There is no CPU path."""
from . import _lib as L
from .action_delay import _steps

MAX_ACTION_HISTORY = 2   # rows of 4: the widest row (20 + 8, and the bias column) still fits the MLP kernels' K = 32 first layer


class ActionHistory:
    """Every observation row ends in the last `rows` (1 or 2) action rows the env was given, most recent first, raw as passed; the hover
    action (1, 0, 0, 0) where the episode is younger.  With `ActionDelay` or `RotorLag` on, these are the commands still in flight.

    >>> env = GpuWaypointEnv(4096, vehicle="quad", action_delay=ActionDelay(0, 2), action_history=ActionHistory(2))   # env.obs_dim == 28
    """

    def __init__(self, rows):
        try:
            self.rows = _steps("rows", rows)
        except L.AmenvError as e:
            raise L.AmenvError(str(e).replace("ActionDelay", "ActionHistory").replace("control steps", "action rows")) from None
        if not 1 <= self.rows <= MAX_ACTION_HISTORY:
            raise L.AmenvError(f"ActionHistory: need 1 <= rows <= {MAX_ACTION_HISTORY}, got {self.rows}")

    def __repr__(self):
        return f"ActionHistory({self.rows})"
