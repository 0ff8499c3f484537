"""Reference side of the actuation-latency tests (include/amenv.h amenv_set_action_delay): numpy and the UNCHANGED
fp64 oracle.

* the d draw restated with the oracle's Philox (the one dr_ref uses): block 0x4C540000 of (seed, global env id, episode), integer arithmetic;
* a numpy history in AGE order: recent[i, k] is the row env i was given k + 1 steps ago in this episode, hover (1, 0, 0, 0) where the
  episode is younger;
* DelayedOracle: the unchanged oracle stepped with the APPLIED rows; hover refill and a redraw wherever it reports AMENV_INFO_WAS_RESET."""
import numpy as np

from oracle import oracle as O

DELAY_BLOCK = 0x4C540000
MAX_DELAY = 8
HOVER = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
WAS_RESET = 128   # AMENV_INFO_WAS_RESET
I_EPISODE = 3     # AMENV_I_EPISODE


def draw(seed, gid, episode, lo, hi):
    """d of one (env, episode): lo + (((w0 >> 16) * (hi - lo + 1)) >> 16)."""
    w0 = int(O.philox(int(seed), int(gid), int(episode) & 0xFFFFFFFF, DELAY_BLOCK)[0])
    return int(lo) + (((w0 >> 16) * (int(hi) - int(lo) + 1)) >> 16)


def draw_all(seed, gid0, episodes, lo, hi):
    """[N] int32 for envs gid0 .. gid0 + N - 1 at their episode counters."""
    return np.array([draw(seed, gid0 + i, int(ep), lo, hi) for i, ep in enumerate(np.asarray(episodes))], np.int32)


class History:
    """d [N] and recent [N, 8, 4] of a batch, kept as the library publishes them."""

    def __init__(self, seed, gid0, episodes, lo, hi):
        self.seed, self.gid0, self.lo, self.hi = int(seed), int(gid0), int(lo), int(hi)
        self.n = len(episodes)
        self.d = draw_all(seed, gid0, episodes, lo, hi)
        self.recent = np.tile(HOVER, (self.n, MAX_DELAY, 1))

    def applied(self, given):
        """[N, 4] f32: what the dynamics get when the envs are given `given`."""
        g = np.asarray(given, np.float32)
        out = g.copy()
        late = self.d > 0
        out[late] = self.recent[np.flatnonzero(late), self.d[late] - 1]
        return out

    def push(self, given, was_reset=None, episodes=None):
        """After the step: the given rows enter; envs whose new episode started (was_reset, with their NEW episode numbers) redraw d and
        get hover rows."""
        self.recent[:, 1:] = self.recent[:, :-1].copy()
        self.recent[:, 0] = np.asarray(given, np.float32)
        if was_reset is not None:
            for i in np.flatnonzero(np.asarray(was_reset)):
                self.restart(i, episodes[i])

    def restart(self, i, episode):
        self.d[i] = draw(self.seed, self.gid0 + int(i), int(episode), self.lo, self.hi)
        self.recent[i] = HOVER


class DelayedOracle:
    """The unchanged oracle flown with the delay, for closed-loop checks on the CPU."""

    def __init__(self, cfg, lo, hi=None):
        self.cfg = cfg
        self.lo, self.hi = int(lo), int(lo if hi is None else hi)
        self.env = O.OracleEnv(cfg)
        self.hist = None

    def reset(self):
        obs = self.env.reset()
        self.hist = History(self.cfg.seed, self.cfg.env_id_offset, self.env.istate[I_EPISODE], self.lo, self.hi)
        return obs

    def step(self, actions):
        """-> the oracle's step dict for the APPLIED rows."""
        a = np.ascontiguousarray(actions, np.float32)
        out = self.env.step(self.hist.applied(a))
        self.hist.push(a, (out["info"] & WAS_RESET) != 0, self.env.istate[I_EPISODE])
        return out
