"""Observation normalisation on the GPU: the equivalent of `VecNormalize(env, norm_obs=True, norm_reward=False)`
that v1/rl_train_vecN.py:10-11 and v1/rl_checkpoint_train_vecN.py:19-26 wrap the env in.

`ObsNormalizer`   -- running mean/var/count of [n, dim] f32 device batches + normalisation (HIP kernels behind
                     amenv_obsnorm_* in include/amenv.h), for GPU-resident loops.
`GpuVecNormalize` -- SB3 `VecNormalize`-shaped wrapper over GpuVecEnv (numpy API): normalises the observations returned
                     by reset()/step_wait() and the `terminal_observation` in infos, `training` flag, `save`/`load`.
                     `norm_reward=True` adds SB3's return-based reward scaling (`RewardNormalizer`, reward_norm.py).
Statistics are saved as .npz (mean, var, count, clip_obs, epsilon, norm_reward and, with it, the return statistics).  The reference's `vec_normalize.pkl` is a pickle of
an SB3 object and is deliberately not read (no unpickling of reference artefacts).  SB3 2.6.0 semantics; parity unpinned.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .reward_norm import RewardNormalizer


class ObsNormalizer:
    def __init__(self, dim, device=0, clip_obs=10.0, epsilon=1e-8):
        self.lib = L.load()
        self.dim, self.clip_obs, self.epsilon = int(dim), float(clip_obs), float(epsilon)
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        h = C.c_void_p()
        rc = self.lib.amenv_obsnorm_create(self.dim, self.device.index, C.byref(h))
        if rc != 0:
            raise L.AmenvError(f"amenv_obsnorm_create failed ({rc}): {self.lib.amenv_last_error(None).decode()}")
        self._h = h

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, obs):
        t = torch.as_tensor(obs)
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        assert t.shape[-1] == self.dim, t.shape
        return t

    def update(self, obs):
        """obs_rms.update(obs): merge this batch's mean / population variance / count."""
        t = self._dev(obs)
        rc = self.lib.amenv_obsnorm_update(self._h, C.c_void_p(t.data_ptr()), t.numel() // self.dim, self._stream())
        if rc != 0:
            raise L.AmenvError(f"amenv_obsnorm_update failed ({rc})")

    def normalize(self, obs, out=None):
        """clip((obs - mean) / sqrt(var + epsilon), -clip_obs, clip_obs) -> new tensor (or `out`, may alias obs)."""
        t = self._dev(obs)
        o = torch.empty_like(t) if out is None else out
        rc = self.lib.amenv_obsnorm_apply(self._h, C.c_void_p(t.data_ptr()), C.c_void_p(o.data_ptr()), t.numel() // self.dim,
                                          self.clip_obs, self.epsilon, self._stream())
        if rc != 0:
            raise L.AmenvError(f"amenv_obsnorm_apply failed ({rc})")
        return o

    def __call__(self, obs, update=True):
        if update:
            self.update(obs)
        return self.normalize(obs)

    def get(self):
        mean, var, count = np.zeros(self.dim), np.zeros(self.dim), np.zeros(1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        if self.lib.amenv_obsnorm_get(self._h, p(mean), p(var), p(count), self._stream()) != 0:
            raise L.AmenvError("amenv_obsnorm_get failed")
        return mean, var, float(count[0])

    def set(self, mean, var, count):
        mean, var = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(var, np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        if self.lib.amenv_obsnorm_set(self._h, p(mean), p(var), float(count), self._stream()) != 0:
            raise L.AmenvError("amenv_obsnorm_set failed")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.amenv_obsnorm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuVecNormalize:
    """`VecNormalize(venv, norm_obs=True, norm_reward=False)` over a GpuVecEnv (same method names as SB3's wrapper).  The default is the
    reference's (v1/rl_train_vecN.py:11); `norm_reward=True` (SB3's own default) divides the rewards by the running standard deviation of
    the discounted returns (`RewardNormalizer`, reward_norm.py): `gamma` is the discount of those returns, `clip_reward` the bound."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=False, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                 normalizer=None, reward_normalizer=None):
        self.venv, self.training, self.norm_obs, self.norm_reward = venv, training, norm_obs, bool(norm_reward)
        self.num_envs, self.observation_space, self.action_space = venv.num_envs, venv.observation_space, venv.action_space
        dim = int(self.observation_space.shape[0])
        dev = getattr(getattr(venv, "backend", None), "device_index", 0)
        self.obs_rms = normalizer if normalizer is not None else ObsNormalizer(dim, dev, clip_obs, epsilon)
        self.ret_rms = None
        if self.norm_reward:
            self.ret_rms = reward_normalizer if reward_normalizer is not None else RewardNormalizer(self.num_envs, gamma, clip_reward, epsilon, dev)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.old_obs = self.old_reward = None

    def _norm(self, obs_np, update):
        self.old_obs = obs_np
        if not self.norm_obs:
            return obs_np
        t = torch.from_numpy(np.ascontiguousarray(obs_np, np.float32))
        if update and self.training:
            self.obs_rms.update(t)
        return self.obs_rms.normalize(t).cpu().numpy()

    def reset(self):
        if self.ret_rms is not None:
            self.ret_rms.reset_returns()
        return self._norm(self.venv.reset(), True)

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rew, done, infos = self.venv.step_wait()
        obs = self._norm(obs, True)
        if self.norm_obs:
            idx = [i for i in np.nonzero(done)[0] if "terminal_observation" in infos[i]]
            if idx:
                t = self.obs_rms.normalize(torch.from_numpy(np.stack([infos[i]["terminal_observation"] for i in idx]).astype(np.float32))).cpu().numpy()
                for k, i in enumerate(idx):
                    infos[i]["terminal_observation"] = t[k]
        self.old_reward = rew
        if self.norm_reward:   # one row of the [T, N] pass; training: the returns advance, join the statistics and restart where done
            rew = self.ret_rms.normalize(torch.from_numpy(np.ascontiguousarray(rew, np.float32)), torch.from_numpy(np.ascontiguousarray(done, np.uint8)),
                                         update=self.training).cpu().numpy()
        return obs, rew, done, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def normalize_obs(self, obs):
        return self.obs_rms.normalize(torch.from_numpy(np.ascontiguousarray(obs, np.float32))).cpu().numpy()

    def get_original_obs(self):
        return self.old_obs

    def normalize_reward(self, reward):
        """clip(reward / sqrt(ret_rms.var + epsilon), -clip_reward, clip_reward) with the current statistics, which do not move (any shape)."""
        if not self.norm_reward:
            return reward
        r = np.ascontiguousarray(reward, np.float32)
        rows = -(-max(r.size, 1) // self.num_envs)
        pad = np.zeros(rows * self.num_envs, np.float32)   # the kernel walks [rows, num_envs] blocks
        pad[:r.size] = r.reshape(-1)
        out = self.ret_rms.normalize(torch.from_numpy(pad.reshape(rows, self.num_envs)), None, update=False).cpu().numpy()
        return out.reshape(-1)[:r.size].reshape(r.shape)

    def get_original_reward(self):
        return self.old_reward

    def save(self, path):
        mean, var, count = self.obs_rms.get()
        extra = {"ret_" + k: v for k, v in self.ret_rms.state_dict().items()} if self.norm_reward else {}
        np.savez(path, mean=mean, var=var, count=count, clip_obs=self.clip_obs, epsilon=self.epsilon, norm_reward=self.norm_reward, **extra)

    @classmethod
    def load(cls, path, venv, normalizer=None, reward_normalizer=None):
        """Statistics written by `save`.  A file from before the return statistics existed loads with norm_reward=False."""
        d = np.load(path if str(path).endswith(".npz") else str(path) + ".npz")
        norm_reward = bool(d["norm_reward"]) if "norm_reward" in d.files else False
        kw = dict(clip_reward=float(d["ret_clip_reward"]), gamma=float(d["ret_gamma"])) if norm_reward else {}
        self = cls(venv, norm_reward=norm_reward, clip_obs=float(d["clip_obs"]), epsilon=float(d["epsilon"]), normalizer=normalizer,
                   reward_normalizer=reward_normalizer, **kw)
        self.obs_rms.set(d["mean"], d["var"], float(d["count"]))
        if norm_reward:
            self.ret_rms.load_state_dict({k[4:]: d[k] for k in d.files if k.startswith("ret_")})
        return self

    def close(self):
        self.obs_rms.close()
        if self.ret_rms is not None:
            self.ret_rms.close()
        self.venv.close()

    def __getattr__(self, name):  # seed, get_attr, env_method, ... fall through to the wrapped env
        return getattr(self.venv, name)
