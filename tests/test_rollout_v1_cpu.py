"""CPU-only checks of the one-launch closed loop with the observation normaliser inside (amenv_rollout_policy_norm): the entry point is
declared, exported and bound, refuses NULL handles before touching a device, and the statistics contract it relies on -- one merge of the
T x N raw rows equals T per-step merges (SB3's RunningMeanStd) -- holds in a numpy restatement."""
import ctypes as C
import os
import re

import numpy as np

import rl_aerial_manipulator_amd as amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1


def test_rollout_policy_norm_is_declared_exported_and_refuses_null_handles():
    hdr = open(os.path.join(ROOT, "include", "amenv.h")).read()
    assert re.search(r"\bint amenv_rollout_policy_norm\s*\(\s*amenv\* env,\s*amenv_obsnorm\* norm,\s*int32_t update,\s*float clip,\s*double eps,", hdr)
    assert "amenv_rollout_policy_norm" in amd._lib.SYMBOLS
    assert hasattr(C.CDLL(amd._lib.LIB_PATH), "amenv_rollout_policy_norm")
    L = amd._lib.load()
    args = (1, 10.0, 1e-8, 8, None, 0, 0) + (None,) * 9
    assert L.amenv_rollout_policy_norm(None, None, *args) == ERR_INVALID
    assert L.amenv_rollout_policy_norm(None, C.c_void_p(16), *args) == ERR_INVALID   # (a normaliser is never dereferenced without an env)
    assert b"non-NULL" in L.amenv_last_error(None)


class RunningMeanStd:
    """stable-baselines3 2.6.0 common/running_mean_std.py, restated (initial mean 0, var 1, count epsilon = 1e-4)."""

    def __init__(self, dim, epsilon=1e-4):
        self.mean, self.var, self.count = np.zeros(dim), np.ones(dim), epsilon

    def update(self, x):
        self.update_from_moments(x.mean(0), x.var(0), x.shape[0])

    def update_from_moments(self, b_mean, b_var, b_count):
        delta, tot = b_mean - self.mean, self.count + b_count
        m2 = self.var * self.count + b_var * b_count + np.square(delta) * self.count * b_count / tot
        self.mean, self.var, self.count = self.mean + delta * b_count / tot, m2 / tot, tot


def test_one_merge_of_all_rows_equals_the_per_step_merges():
    """Chan's parallel-moments merge is associative: the launch's single merge of rows 1..T of every env (batch count T x N) gives the
    statistics T per-step VecNormalize updates give, to fp64 rounding -- also for nearly constant columns and a drifting mean."""
    rng = np.random.RandomState(3)
    T, n, d = 64, 512, 17
    scale = np.array([10.0, 0.5, 1e-3] + [1.0] * (d - 3))
    rows = rng.normal(size=(T, n, d)) * scale + np.linspace(0.0, 4.0, T)[:, None, None] * (np.arange(d) % 3 == 0)
    rows[..., 5] = 1.0 + 1e-4 * rng.normal(size=(T, n))               # quaternion-w-like column: var ~ 1e-8
    warm = rng.normal(size=(n, d))
    a, b = RunningMeanStd(d), RunningMeanStd(d)
    a.update(warm); b.update(warm)
    for t in range(T):
        a.update(rows[t])
    flat = rows.reshape(T * n, d)
    s1, s2 = flat.sum(0), (flat * flat).sum(0)                          # the kernel's fp64 column sums, then obsnorm_merge_kernel's moments
    b_mean = s1 / (T * n)
    b.update_from_moments(b_mean, np.maximum(s2 / (T * n) - b_mean * b_mean, 0.0), T * n)
    assert np.isclose(a.count, 1e-4 + n + T * n, rtol=1e-15, atol=0) and b.count == (1e-4 + n) + T * n
    np.testing.assert_allclose(b.mean, a.mean, rtol=1e-12, atol=1e-14)
    # var: the sum-of-squares form loses |mean|^2 / var digits on the near-constant column (the same form amenv_obsnorm_update uses)
    np.testing.assert_allclose(b.var, a.var, rtol=1e-12, atol=1e-14 * float(np.max(b.mean ** 2 + b.var)))
    two_pass = RunningMeanStd(d)
    two_pass.update(warm)
    two_pass.update(flat)
    np.testing.assert_allclose(two_pass.mean, a.mean, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(two_pass.var, a.var, rtol=1e-12, atol=1e-14 * float(np.max(a.mean ** 2 + a.var)))
