"""fp64 numpy restatement of the reward half of SB3 2.6.0's VecNormalize (common/vec_normalize.py: step_wait / _update_reward /
normalize_reward; common/running_mean_std.py), third-party semantics, parity unpinned.  The checker of the GPU reward normaliser:
two-pass np.mean / np.var per step, `returns[done] = 0` after the step's rewards are normalised."""
import numpy as np


class RetNormRef:
    def __init__(self, num_envs, gamma=0.99, clip_reward=10.0, epsilon=1e-8):
        self.n, self.gamma, self.clip, self.eps = int(num_envs), float(gamma), float(clip_reward), float(epsilon)
        self.mean, self.var, self.count = 0.0, 1.0, 1e-4        # RunningMeanStd(shape=()) defaults
        self.returns = np.zeros(self.n, np.float64)

    def reset(self):
        self.returns = np.zeros(self.n, np.float64)

    def _update(self, arr):                                     # RunningMeanStd.update -> update_from_moments
        bm, bv, bc = float(np.mean(arr)), float(np.var(arr)), arr.shape[0]
        delta = bm - self.mean
        tot = self.count + bc
        m2 = self.var * self.count + bv * bc + np.square(delta) * self.count * bc / tot
        self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / tot, tot

    def step(self, r, done, update=True):
        """One env step: r [N] float32 raw rewards, done [N] -> normalised rewards [N] float64 (compare after a cast to float32)."""
        r64 = np.asarray(r, np.float32).astype(np.float64)
        if update:
            self.returns = self.returns * self.gamma + r64
            self._update(self.returns)
        out = np.clip(r64 / np.sqrt(self.var + self.eps), -self.clip, self.clip)
        if update:
            self.returns[np.asarray(done).astype(bool)] = 0.0
        return out

    def block(self, rewards, dones, update=True):
        """[T, N] rewards and dones, one step after the other."""
        return np.stack([self.step(rewards[t], dones[t], update) for t in range(rewards.shape[0])])

    def state(self):
        return self.mean, self.var, self.count, self.returns.copy()


def make_block(T, N, seed):
    """The test inputs: rewards 300 + N(0, 1) with +-400 spikes at ~2 % of the entries (the offset stresses cancellation in the variance),
    dones Bernoulli(0.1) plus forced episode ends at t = 0 and t = T - 1."""
    rng = np.random.RandomState(seed)
    r = 300.0 + rng.normal(size=(T, N))
    spike = rng.rand(T, N) < 0.02
    r = np.where(spike, r + rng.choice([-400.0, 400.0], size=(T, N)), r).astype(np.float32)
    d = (rng.rand(T, N) < 0.1).astype(np.uint8)
    d[0, rng.randint(N)] = 1
    d[T - 1, rng.randint(N)] = 1
    return r, d
