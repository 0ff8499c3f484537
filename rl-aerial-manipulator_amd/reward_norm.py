"""Reward normalisation on the GPU: the reward half of SB3's `VecNormalize(env, norm_reward=True)` (its default; the
reference's own set-up turns it off, v1/rl_train_vecN.py:11).

`RewardNormalizer` holds, on the device, the discounted return of every env (`returns[N]`, fp64) and ONE running
mean / population variance / count of those returns (initial 0 / 1 / 1e-4).  Per env step t, training:
    returns = returns * gamma + r_t ;  ret_rms.update(returns) ;  out_t = clip(r_t / sqrt(ret_rms.var + epsilon), +-clip_reward) ;
    returns[done_t] = 0
Normalised rewards never feed back into a rollout, so a whole time-major [T, N] block of raw rewards and dones is processed after
the fact in one call (HIP kernels behind amenv_retnorm_* in include/amenv.h, csrc/amenv_retnorm.hpp) with exactly the per-step
result: T calls of one step, one call of T steps and any other split give the same bytes.  `update=False` freezes the statistics
and the returns (evaluation).  SB3 2.6.0 semantics restated; parity unpinned, checked against a numpy restatement.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


class RewardNormalizer:
    def __init__(self, num_envs, gamma=0.99, clip_reward=10.0, epsilon=1e-8, device=0):
        self.lib = L.load()
        self.num_envs, self.gamma, self.clip_reward, self.epsilon = int(num_envs), float(gamma), float(clip_reward), float(epsilon)
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        h = C.c_void_p()
        rc = self.lib.amenv_retnorm_create(self.num_envs, self.gamma, self.device.index, C.byref(h))
        if rc != 0:
            raise L.AmenvError(f"amenv_retnorm_create failed ({rc}): {self.lib.amenv_last_error(None).decode()}")
        self._h = h

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def normalize(self, rewards, dones, out=None, update=True):
        """rewards [N] or [T, N] f32 and dones (same shape, u8 / bool: the episode ended AT that step) on the device -> the
        normalised rewards in a new tensor (or `out`, which may be `rewards`).  update=True advances returns and statistics step
        by step as a training VecNormalize does; update=False scales with the current variance and changes nothing (dones may be None)."""
        r = torch.as_tensor(rewards)
        if r.device != self.device or r.dtype != torch.float32 or not r.is_contiguous():
            r = r.to(device=self.device, dtype=torch.float32).contiguous()
        if r.dim() not in (1, 2) or r.shape[-1] != self.num_envs or r.numel() == 0:
            raise L.AmenvError(f"RewardNormalizer.normalize: rewards must be [{self.num_envs}] or [T, {self.num_envs}], got {tuple(r.shape)}")
        d = None
        if dones is not None:
            d = torch.as_tensor(dones)
            if d.dtype == torch.bool:
                d = d.to(torch.uint8)
            if d.device != self.device or d.dtype != torch.uint8 or not d.is_contiguous():
                d = d.to(device=self.device, dtype=torch.uint8).contiguous()
            if d.shape != r.shape:
                raise L.AmenvError(f"RewardNormalizer.normalize: dones {tuple(d.shape)} != rewards {tuple(r.shape)}")
        elif update:
            raise L.AmenvError("RewardNormalizer.normalize: update=True needs the dones")
        o = torch.empty_like(r) if out is None else out
        if o.shape != r.shape or o.dtype != torch.float32 or o.device != self.device or not o.is_contiguous():
            raise L.AmenvError("RewardNormalizer.normalize: out must be a contiguous float32 device tensor of the rewards' shape")
        rc = self.lib.amenv_retnorm_rollout(self._h, r.numel() // self.num_envs, C.c_void_p(r.data_ptr()), None if d is None else C.c_void_p(d.data_ptr()),
                                            C.c_void_p(o.data_ptr()), 1 if update else 0, self.clip_reward, self.epsilon, self._stream())
        if rc != 0:
            raise L.AmenvError(f"amenv_retnorm_rollout failed ({rc}): {self.lib.amenv_last_error(None).decode()}")
        return o

    def reset_returns(self):
        """`VecNormalize.reset()`: the returns start from zero, the statistics stay."""
        if self.lib.amenv_retnorm_reset_returns(self._h, self._stream()) != 0:
            raise L.AmenvError("amenv_retnorm_reset_returns failed")

    def get(self):
        """(mean, var, count, returns[N]) as host values."""
        m, v, c = C.c_double(), C.c_double(), C.c_double()
        ret = np.zeros(self.num_envs, np.float64)
        if self.lib.amenv_retnorm_get(self._h, C.byref(m), C.byref(v), C.byref(c), ret.ctypes.data_as(C.c_void_p), self._stream()) != 0:
            raise L.AmenvError("amenv_retnorm_get failed")
        return m.value, v.value, c.value, ret

    def set(self, mean, var, count, returns=None):
        """Install statistics and, unless None, the returns."""
        p = None
        if returns is not None:
            returns = np.ascontiguousarray(returns, np.float64)
            if returns.shape != (self.num_envs,):
                raise L.AmenvError(f"RewardNormalizer.set: returns must be [{self.num_envs}], got {returns.shape}")
            p = returns.ctypes.data_as(C.c_void_p)
        if self.lib.amenv_retnorm_set(self._h, float(mean), float(var), float(count), p, self._stream()) != 0:
            raise L.AmenvError("amenv_retnorm_set failed (mean / var / count must be finite, var >= 0, count > 0)")

    def state_dict(self):
        """Plain numpy: the statistics, the carried returns and the three constants."""
        mean, var, count, returns = self.get()
        f = lambda x: np.array(x, np.float64)  # noqa: E731
        return dict(mean=f(mean), var=f(var), count=f(count), returns=returns, gamma=f(self.gamma), clip_reward=f(self.clip_reward), epsilon=f(self.epsilon))

    def load_state_dict(self, sd):
        if float(sd["gamma"]) != self.gamma:
            raise L.AmenvError(f"RewardNormalizer.load_state_dict: saved with gamma={float(sd['gamma'])}, this one has gamma={self.gamma}")
        returns = np.asarray(sd["returns"], np.float64) if "returns" in sd else None
        if returns is not None and returns.shape != (self.num_envs,):   # another number of envs: the statistics carry over, the returns restart
            returns = np.zeros(self.num_envs, np.float64)
        self.clip_reward, self.epsilon = float(sd["clip_reward"]), float(sd["epsilon"])
        self.set(float(sd["mean"]), float(sd["var"]), float(sd["count"]), returns)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.amenv_retnorm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
