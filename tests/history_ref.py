"""Reference side of the action-history tests (include/amenv.h amenv_set_action_history): numpy on top of
tests/delay_ref.py, which it imports unchanged.

* rows(hist, H): the 4 H columns an observation row ends with -- the first H rows of a delay_ref.History, most recent first;
* HistoryOracle: delay_ref.DelayedOracle (range (0, 0) when there is no delay) whose observation rows carry those columns.  A terminal
  row is formed BEFORE the hover refill (it ends in [a_t, a_{t-1}] of the episode that ended), the row of a new episode after it."""
import numpy as np

from tests import delay_ref


def rows(hist, H):
    """[N, 4 H] f32: hist.recent[:, :H], row k = the row given k + 1 steps ago."""
    return np.ascontiguousarray(hist.recent[:, :H]).reshape(hist.n, 4 * H).astype(np.float32)


def pushed(hist, given, H):
    """[N, 4 H] f32: what rows() returns after `given` has entered and before any refill -- the columns of this step's rows of the envs
    that go on, and of the terminal rows."""
    r = np.concatenate([np.asarray(given, np.float32)[:, None], hist.recent[:, :-1]], axis=1)
    return np.ascontiguousarray(r[:, :H]).reshape(hist.n, 4 * H).astype(np.float32)


class HistoryOracle:
    """The unchanged oracle flown with the delay (or without: range (0, 0)) and the history appended to its rows."""

    def __init__(self, cfg, H, lo=0, hi=None):
        self.H = int(H)
        self.inner = delay_ref.DelayedOracle(cfg, lo, hi)

    @property
    def env(self):
        return self.inner.env

    @property
    def hist(self):
        return self.inner.hist

    def reset(self):
        obs = self.inner.reset()
        return np.concatenate([obs, rows(self.hist, self.H).astype(obs.dtype)], axis=1)

    def step(self, actions):
        """-> the oracle's step dict; "obs" widened (hover columns where a new episode started) and "terminal_hist" [N, 4 H]: the columns a
        terminal row of this step ends with."""
        a = np.ascontiguousarray(actions, np.float32)
        term = pushed(self.hist, a, self.H)
        out = dict(self.inner.step(a))
        out["terminal_hist"] = term
        out["obs"] = np.concatenate([out["obs"], rows(self.hist, self.H).astype(out["obs"].dtype)], axis=1)
        return out
