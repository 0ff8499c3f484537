"""GPU-resident PPO over `GpuWaypointEnv` (BASELINE config 5).

Mirrors what the reference's training entry does through Stable-Baselines3 (v2/rl_train.py:22-56):
`PPO("MlpPolicy", env, learning_rate=2e-4, n_steps=2048, batch_size=128, n_epochs=12, gamma=.995, gae_lambda=.9,
clip_range=.2, ent_coef=5e-4, policy_kwargs=dict(net_arch=[128,64,64], activation_fn=nn.Tanh))` and SB3's defaults
(vf_coef .5, max_grad_norm .5, normalize_advantage, Adam eps 1e-5, orthogonal init; values read from the `data` JSON of
`checkpoints_from_8_6M/ppo_model_2300000_steps.zip`).  SB3 2.6.0 is third-party and absent here: its published algorithm is
restated, **parity unpinned** except for the policy network itself, whose tensors load from the reference's `policy.pth`
(tests: the reference's best checkpoint flies the waypoint task on this env).

What runs where:
  * env step, GAE (`amenv_gae`), action sampling + log-prob + clip (`amenv_gaussian_act`): HIP kernels behind the C ABI;
  * the two 20->128->64->64 tanh MLPs, their backward and Adam: PyTorch-ROCm (rocBLAS GEMMs) -- plumbing, as SURVEY §1 says;
  * the whole rollout stays in HBM: the env writes obs / reward / done straight into rows of the rollout buffer;
  * multi-GPU: one process per GPU, envs sharded by global id, ONE all-reduce per minibatch of one flat fp32 gradient buffer
    (30,537 parameters = 122 KB for the 20-D / 4-D task) over RCCL; nothing on the step path.
"""
import ctypes as C
import io
import json
import math
import os
import zipfile

import numpy as np
import torch
from torch import nn

from . import _lib as L


_SPLIT = int(os.environ.get("AMENV_PPO_SPLIT", "1024"))   # rows per partial product of the weight gradient (measured: 128..2048 within 5 %, 1024 best)


class _TallSkinnyLinearFn(torch.autograd.Function):
    """y = x W^T + b with a weight gradient shaped for this workload.  dW = dY^T X is a [out, in] <= 128 x 128 result
    reduced over the whole minibatch (65,536 rows): the library GEMM picked for that shape runs in one or two workgroups
    without split-K (rocprof, profiles/r01/ppo_update_kernel_stats_before.csv: ~200 us per call, 55 % of the update).
    Here the batch is cut into 1024-row slabs (256 for small batches), one strided-batched GEMM forms the per-slab products on all CUs and a sum
    over slabs finishes the reduction."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy @ w if ctx.needs_input_grad[0] else None
        rows = x.shape[0]
        split = _SPLIT if rows >= 2 * _SPLIT else 256
        c = rows // split
        m = c * split
        gw = torch.bmm(gy[:m].view(c, split, -1).transpose(1, 2), x[:m].view(c, split, -1)).sum(0)
        if m < rows:
            gw = gw + gy[m:].t() @ x[m:]
        return gx, gw, gy.sum(0)


class _Linear(nn.Linear):
    """nn.Linear (same parameters and state-dict keys) that switches to the tall-skinny weight gradient for big batches."""

    def forward(self, x):
        if x.dim() == 2 and x.shape[0] >= 512 and torch.is_grad_enabled() and x.is_contiguous():
            return _TallSkinnyLinearFn.apply(x, self.weight, self.bias)
        return super().forward(x)


def _mlp(sizes):
    layers = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        layers += [_Linear(a, b), nn.Tanh()]
    return nn.Sequential(*layers)


class _MlpExtractor(nn.Module):
    """Separate actor / critic trunks; attribute names give SB3's state-dict keys `mlp_extractor.policy_net.{0,2,4}.*`."""

    def __init__(self, obs_dim, net_arch):
        super().__init__()
        self.policy_net = _mlp([obs_dim, *net_arch])
        self.value_net = _mlp([obs_dim, *net_arch])


class ActorCritic(nn.Module):
    """SB3 `ActorCriticPolicy` for a Box action space: tanh MLP [128,64,64] x2, linear heads, state-independent log_std
    (v2/rl_train.py:27-30).  `state_dict()` has exactly the keys and shapes of the reference checkpoints' `policy.pth`."""

    def __init__(self, obs_dim=20, act_dim=4, net_arch=(128, 64, 64), log_std_init=0.0, ortho_init=True,
                 action_low=None, action_high=None):
        super().__init__()
        self.obs_dim, self.act_dim, self.net_arch = int(obs_dim), int(act_dim), tuple(net_arch)
        self.log_std = nn.Parameter(torch.full((self.act_dim,), float(log_std_init)))
        self.mlp_extractor = _MlpExtractor(self.obs_dim, self.net_arch)
        self.action_net = _Linear(self.net_arch[-1], self.act_dim)
        self.value_net = _Linear(self.net_arch[-1], 1)
        # action space of WaypointQuadEnv (v2/rl_env_scaledObs.py:20-24); joint commands of the arm are in [-1, 1] too
        lo = [0.0] + [-1.0] * (self.act_dim - 1) if action_low is None else action_low
        hi = [2.0] + [1.0] * (self.act_dim - 1) if action_high is None else action_high
        self.register_buffer("action_low", torch.as_tensor(lo, dtype=torch.float32), persistent=False)
        self.register_buffer("action_high", torch.as_tensor(hi, dtype=torch.float32), persistent=False)
        if ortho_init:  # SB3: gain sqrt(2) for the trunks, 0.01 for the action head, 1 for the value head
            for mod, gain in ((self.mlp_extractor, math.sqrt(2.0)), (self.action_net, 0.01), (self.value_net, 1.0)):
                for m in mod.modules():
                    if isinstance(m, nn.Linear):
                        nn.init.orthogonal_(m.weight, gain=gain)
                        nn.init.zeros_(m.bias)
        self.flat_param = self.flat_grad = None

    # ---- forward pieces -----------------------------------------------------------------------
    _FUSED_DIMS = {(20, 4), (29, 7), (17, 4), (25, 5), (27, 6),   # v2 | hexacopter + 3-link arm | v1 | + 1- / 2-link arm
                   (24, 4), (28, 4), (21, 4), (25, 4)}            # v2 / v1 rows with one or two action rows of history (ActionHistory)
    MFMA_FORWARD_ROWS = 8192   # batches from here on take amenv_policy_forward_mfma (below: the VALU kernel's shorter latency wins)

    def fused_ok(self, obs):
        """The one-launch HIP forward (`amenv_policy_forward`) applies: inference on the GPU, parameters in the flat buffer,
        the reference's architecture.  Training passes (autograd) go through the torch modules."""
        return (self.flat_param is not None and self.flat_param.data_ptr() == self.log_std.data_ptr()   # still the parameters' home
                and obs.is_cuda and obs.device == self.flat_param.device and not torch.is_grad_enabled() and self.net_arch == (128, 64, 64)
                and (self.obs_dim, self.act_dim) in self._FUSED_DIMS and obs.dtype == torch.float32 and obs.dim() == 2)

    def forward_fused(self, obs, want_mean=True, want_value=True):
        """mean [n, A] and / or value [n] of a batch of observations in ONE kernel launch (weights as scalar operands of the FMAs,
        activations through LDS; csrc/amenv_policy.hpp) instead of 14 library kernels; large batches on the matrix cores (two launches)."""
        obs = obs.contiguous()
        n = obs.shape[0]
        mean = torch.empty(n, self.act_dim, dtype=torch.float32, device=obs.device) if want_mean else None
        value = torch.empty(n, dtype=torch.float32, device=obs.device) if want_value else None
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        if n >= self.MFMA_FORWARD_ROWS:   # large batches: the training kernel's forward passes (matrix cores, csrc/amenv_mlp_train.hpp)
            ws = self.__dict__.get("_fwd_ws")
            if ws is None or ws.device != obs.device:
                ws = self.__dict__["_fwd_ws"] = torch.empty(L.load().amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device=obs.device)
            rc = L.load().amenv_policy_forward_mfma(p(self.flat_param.detach()), self.obs_dim, self.act_dim, p(obs), n, p(mean), p(value), p(ws), stream)
        else:
            rc = L.load().amenv_policy_forward(p(self.flat_param.detach()), self.obs_dim, self.act_dim, p(obs), n, p(mean), p(value), stream)
        if rc != 0:
            raise L.AmenvError(f"amenv_policy_forward failed ({rc})")
        return mean, value

    def actor(self, obs):
        if self.fused_ok(obs):
            return self.forward_fused(obs, True, False)[0]
        return self.action_net(self.mlp_extractor.policy_net(obs))

    def critic(self, obs):
        if self.fused_ok(obs):
            return self.forward_fused(obs, False, True)[1]
        return self.value_net(self.mlp_extractor.value_net(obs)).squeeze(-1)

    def actor_critic(self, obs):
        """mean, value -- one launch on the GPU inference path."""
        if self.fused_ok(obs):
            return self.forward_fused(obs, True, True)
        return self.actor(obs), self.critic(obs)

    def evaluate_actions(self, obs, actions):
        """values, log pi(a|s), entropy -- SB3 ActorCriticPolicy.evaluate_actions for DiagGaussianDistribution."""
        mean = self.actor(obs)
        z = (actions - mean) * torch.exp(-self.log_std)
        logp = (-0.5 * z * z - self.log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + self.log_std).sum().expand(obs.shape[0])
        return self.critic(obs), logp, entropy

    @torch.no_grad()
    def predict(self, obs, deterministic=True, generator=None):
        """Action for the env: mean (or a sample) clipped to the action space, as SB3's `policy.predict`."""
        if obs.is_cuda and (self.flat_param is None or self.flat_param.data_ptr() != self.log_std.data_ptr()):
            self.flatten_()          # inference on the GPU goes through the one-launch forward, which reads the flat buffer
        mean = self.actor(obs)
        if not deterministic:
            mean = mean + torch.exp(self.log_std) * torch.randn(mean.shape, device=mean.device, generator=generator)
        return torch.minimum(torch.maximum(mean, self.action_low), self.action_high)

    # ---- one flat parameter / gradient buffer ---------------------------------------------------
    def flatten_(self):
        """Re-home every parameter (and its gradient) as a view into ONE flat fp32 buffer: the optimiser updates one
        tensor and the multi-GPU gradient exchange is one all-reduce of `flat_grad`."""
        ps = list(self.parameters())
        n = sum(p.numel() for p in ps)
        flat = torch.empty(n, dtype=ps[0].dtype, device=ps[0].device)
        grad = torch.zeros_like(flat)
        off = 0
        for p in ps:
            k = p.numel()
            flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = flat[off:off + k].view_as(p)
            p.grad = grad[off:off + k].view_as(p)
            off += k
        self.flat_param, self.flat_grad = flat, grad
        if flat.is_cuda and (self.obs_dim, self.act_dim) in self._FUSED_DIMS and self.net_arch == (128, 64, 64):
            # workspace of the matrix-core forward (forward_fused, large batches): allocated here, never inside a graph capture
            self.__dict__["_fwd_ws"] = torch.empty(L.load().amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device=flat.device)
        return self

    def num_parameters(self):
        return sum(p.numel() for p in self.parameters())

    # ---- SB3 checkpoint tensors -------------------------------------------------------------------
    @staticmethod
    def read_sb3_state_dict(path):
        """Tensors of an SB3 checkpoint: a `.zip` as `PPO.save` writes (v2/rl_train.py:57, `policy.pth` inside) or a bare
        `policy.pth`.  Loaded with `weights_only=True`: nothing from the file is executed."""
        if zipfile.is_zipfile(path):
            with zipfile.ZipFile(path) as z:
                names = z.namelist()
                if "policy.pth" in names:
                    return torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
        return torch.load(path, weights_only=True, map_location="cpu")

    @classmethod
    def from_sb3(cls, path_or_state_dict, device="cpu"):
        sd = path_or_state_dict if isinstance(path_or_state_dict, dict) else cls.read_sb3_state_dict(path_or_state_dict)
        w0 = sd["mlp_extractor.policy_net.0.weight"]
        arch = tuple(int(sd[f"mlp_extractor.policy_net.{i}.weight"].shape[0]) for i in range(0, 64, 2)
                     if f"mlp_extractor.policy_net.{i}.weight" in sd)
        pol = cls(obs_dim=int(w0.shape[1]), act_dim=int(sd["action_net.weight"].shape[0]), net_arch=arch, ortho_init=False)
        pol.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
        return pol.to(device)

    def save_sb3_policy(self, path):
        """Write `policy.pth` with SB3's key names: `model.policy.load_state_dict(torch.load(path))` accepts it."""
        torch.save({k: v.detach().cpu().clone() for k, v in self.state_dict().items()}, path)


class RolloutBuffer:
    """Time-major rollout storage in HBM: obs [T+1, N, D] (row T = the observation after the last step), raw actions
    [T, N, A], log-probs / values / rewards / advantages / returns [T, N] f32, dones [T, N] u8 (episode ended AT step t)."""

    def __init__(self, n_steps, n_envs, obs_dim, act_dim, device):
        T, N = int(n_steps), int(n_envs)
        f = dict(dtype=torch.float32, device=device)
        self.n_steps, self.n_envs = T, N
        self.obs = torch.zeros(T + 1, N, obs_dim, **f)
        self.actions = torch.zeros(T, N, act_dim, **f)
        self.logp = torch.zeros(T, N, **f)
        self.values = torch.zeros(T, N, **f)
        self.rewards = torch.zeros(T, N, **f)
        self.dones = torch.zeros(T, N, dtype=torch.uint8, device=device)
        self.last_values = torch.zeros(N, **f)
        self.advantages = torch.zeros(T, N, **f)
        self.returns = torch.zeros(T, N, **f)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in vars(self).values() if torch.is_tensor(t))


def explained_variance(values, returns):
    """SB3 `explained_variance(y_pred = values, y_true = returns)`: 1 - Var[returns - values] / Var[returns] (population variances) as a
    0-dim tensor on the inputs' device; 0.0 where SB3 gives NaN (constant returns), so that a log record stays finite."""
    y, v = returns.reshape(-1).to(torch.float64), values.reshape(-1).to(torch.float64)
    var_y = y.var(unbiased=False)
    ev = 1.0 - (y - v).var(unbiased=False) / torch.where(var_y > 0, var_y, torch.ones_like(var_y))
    return torch.where(var_y > 0, ev, torch.zeros_like(ev)).to(torch.float32)


def compute_gae(buffer, gamma, gae_lambda):
    """advantages / returns of a rollout buffer through the HIP kernel (`amenv_gae`); device tensors only."""
    b = buffer
    if not b.rewards.is_cuda:
        raise L.AmenvError("compute_gae runs on the GPU only (amenv_gae); there is no CPU fallback")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.load().amenv_gae(p(b.rewards), p(b.values), p(b.dones), p(b.last_values), p(b.advantages), p(b.returns),
                            b.n_steps, b.n_envs, float(gamma), float(gae_lambda),
                            C.c_void_p(torch.cuda.current_stream(b.rewards.device).cuda_stream))
    if rc != 0:
        raise L.AmenvError(f"amenv_gae failed ({rc})")
    return b.advantages, b.returns


def gaussian_act(mean, log_std, low, high, raw_out, clipped_out, logp_out, seed, draw, env_id_offset=0):
    """Sample + log-prob + clip in one launch (`amenv_gaussian_act`); noise keyed by (seed, global env id, draw)."""
    if not mean.is_cuda:
        raise L.AmenvError("gaussian_act runs on the GPU only (amenv_gaussian_act); there is no CPU fallback")
    n, a = mean.shape
    for t in (mean, raw_out, clipped_out, logp_out, log_std, low, high):
        if not (t.is_contiguous() and t.dtype == torch.float32 and t.device == mean.device):
            raise L.AmenvError("gaussian_act: contiguous float32 tensors on one device required")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.load().amenv_gaussian_act(p(mean), p(log_std), p(low), p(high), p(raw_out), p(clipped_out), p(logp_out), n, a,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, int(env_id_offset),
                                     C.c_void_p(torch.cuda.current_stream(mean.device).cuda_stream))
    if rc != 0:
        raise L.AmenvError(f"amenv_gaussian_act failed ({rc}): act_dim must be 4..7")


class KlAdaptiveLr:
    """The KL-adaptive learning rate of the GPU-parallel PPO implementations (rsl_rl's rule and defaults), driven by every
    minibatch's `approx_kl` (SB3's estimator):

        if      kl > band * desired_kl:           lr = max(lr / factor, lr_min)
        else if kl > 0 and kl < desired_kl / band: lr = min(lr * factor, lr_max)
        else                                       lr unchanged                   (a NaN kl: unchanged)

    A plain value class.  `step(lr, kl)` IS the rule, in numpy.float32 -- the arithmetic of `amenv_ppo_adam_step_adapt`, bit for bit; the
    host update paths call it, the fused path hands `struct()` to the kernel.  The value checks are the C ABI's."""
    FIELDS = ("desired_kl", "factor", "band", "lr_min", "lr_max")

    def __init__(self, desired_kl=0.01, factor=1.5, band=2.0, lr_min=1e-5, lr_max=1e-2):
        try:
            v = [np.float32(x) for x in (desired_kl, factor, band, lr_min, lr_max)]
        except (TypeError, ValueError) as e:
            raise L.AmenvError(f"KlAdaptiveLr: five numbers expected ({e})") from None
        self.desired_kl, self.factor, self.band, self.lr_min, self.lr_max = v
        if not all(np.isfinite(x) for x in v):
            raise L.AmenvError(f"KlAdaptiveLr: every value must be finite in float32 (got {self!r})")
        if not (self.desired_kl > 0 and self.band >= 1 and self.factor > 1 and 0 < self.lr_min <= self.lr_max):
            raise L.AmenvError(f"KlAdaptiveLr needs desired_kl > 0, band >= 1, factor > 1 and 0 < lr_min <= lr_max (got {self!r})")

    def step(self, lr, kl):
        """The learning rate after a minibatch whose approx_kl is `kl`, as numpy.float32."""
        lr, kl = np.float32(lr), np.float32(kl)
        if kl > self.band * self.desired_kl:
            return np.maximum(lr / self.factor, self.lr_min)
        if kl > 0 and kl < self.desired_kl / self.band:
            return np.minimum(lr * self.factor, self.lr_max)
        return lr

    def struct(self):
        return L.PpoLrRule(C.sizeof(L.PpoLrRule), float(self.desired_kl), float(self.band), float(self.factor), float(self.lr_min), float(self.lr_max))

    def state_dict(self):
        """The five numbers as Python floats (each holds its float32 exactly: JSON brings them back bit for bit)."""
        return {k: float(getattr(self, k)) for k in self.FIELDS}

    def __eq__(self, other):
        return isinstance(other, KlAdaptiveLr) and self.state_dict() == other.state_dict()

    def __repr__(self):
        return "KlAdaptiveLr(" + ", ".join(f"{k}={float(getattr(self, k))!r}" for k in self.FIELDS) + ")"


class MinibatchStep:
    """One PPO minibatch update (SB3 `PPO.train` inner loop body): loss, backward, gradient exchange, clip, Adam.

    On the GPU the step is launch-bound in eager mode (~200 small kernels per minibatch; rocprof: 245 ms of kernels in a
    359 ms update), so after three eager calls it is captured into HIP graphs on static minibatch buffers and replayed:
    one graph for a single GPU; for several GPUs two graphs (forward/backward | clip + Adam) around the ONE eager RCCL
    all-reduce of the flat gradient buffer.  A ragged last minibatch (n % batch_size) always runs eagerly.

    `stats` (device, 5 floats): policy loss, value loss, entropy loss, clip fraction, gradient norm of the last minibatch; `kl` (device,
    1 float): its approx_kl -- on the HIP paths a view of the control block's `kl_last`, which is where the kernels put it.

    `target_kl` (SB3's: leave the update once a minibatch's approx_kl exceeds 1.5 target_kl, after its loss and before its optimiser
    step).  Where the whole step is HIP (fused MLP + fused Adam) the decision is taken and obeyed ON THE DEVICE through the
    control block `amenv_ppo_ctl`: no host synchronisation, the caller keeps launching and the kernels of the later minibatches return at
    entry (`device_gate`).  Every other path checks on the host like SB3, one synchronisation per minibatch, and sets `stopped`.  Captured
    graphs are not built with it (`use_graph=True` raises), nor are several ranks (they would disagree on the stop).  `arm()` starts an
    update: it zeroes the counters and re-opens the gate; `ppo_update` calls it.

    `set_hyper(learning_rate, clip_range)`: new values for the next minibatches (the schedules of `PPO`).  The fused Adam step re-uploads
    its hyper-parameters when they change and the eager paths read them on every call; CAPTURED GRAPHS have `clip_range` baked in (a launch
    argument) and, with torch's Adam, the learning rate too: such a change drops them and the next full minibatch captures again (one
    capture per change, i.e. per iteration under a schedule).  With the fused Adam step the learning rate lives in a device buffer that the
    replayed launch reads, so a change of the learning rate alone is one small upload and the graphs stay.

    `adaptive_lr` (a `KlAdaptiveLr`): the learning rate follows every minibatch's approx_kl, in the gate's order -- loss ->
    approx_kl -> (stop?) -> rule -> optimiser step with the new rate; after a stop nothing moves.  Where the whole step is HIP the rule runs
    ON THE DEVICE (`amenv_ppo_adam_step_adapt`, `device_rule`): the rate lives in `hyper6[0]`, which the host uploads before an update's first
    step and then leaves alone; `readout` brings it back with the update's one transfer and writes it to `param_groups[0]["lr"]`.  Every
    other path runs `KlAdaptiveLr.step` on the host after the loss, one synchronisation per minibatch, and sets `param_groups[0]["lr"]`.
    Refused with captured graphs and with several ranks, as `target_kl` is and for its reasons.

    `clip_range_vf` (SB3's clipped value loss; None = off): v_pred = v_old + clamp(v - v_old, -c, c).  The step then takes the rollout's old
    values as a sixth tensor (`old_values`); the HIP paths launch the `_vclip` entry points, the torch path states the same formula."""

    def __init__(self, policy, optimizer, *, clip_range=0.2, ent_coef=5e-4, vf_coef=0.5, max_grad_norm=0.5,
                 normalize_advantage=True, dist=None, use_graph=None, split_graphs=None, fused_loss=None, fused_mlp=None, target_kl=None,
                 adaptive_lr=None, clip_range_vf=None):
        if policy.flat_grad is None:
            policy.flatten_()
        self.policy, self.optimizer, self.dist = policy, optimizer, dist
        self.world = dist.get_world_size() if dist is not None else 1
        if adaptive_lr is not None and not isinstance(adaptive_lr, KlAdaptiveLr):
            raise L.AmenvError(f"adaptive_lr must be a KlAdaptiveLr or None (got {type(adaptive_lr).__name__})")
        self.adaptive_lr = adaptive_lr
        if adaptive_lr is not None:
            if self.world > 1:
                raise L.AmenvError("adaptive_lr with several ranks is not built: every rank would move its learning rate by its own shard's approx_kl and "
                                   "the ranks would step with different rates; train with adaptive_lr=None")
            if use_graph:
                raise L.AmenvError("adaptive_lr with use_graph=True is not built: the rule sits between the loss and the optimiser step, inside "
                                   "what a captured graph replays as one piece; leave use_graph unset (adaptive_lr runs the eager paths)")
            use_graph = False
        self.clip_range_vf = None if clip_range_vf is None else float(clip_range_vf)
        if self.clip_range_vf is not None and not (self.clip_range_vf > 0.0 and math.isfinite(self.clip_range_vf)):
            raise L.AmenvError(f"clip_range_vf must be positive and finite (got {clip_range_vf!r}); None switches the value clip off")
        self.target_kl = None if target_kl is None else float(target_kl)
        if self.target_kl is not None:
            if not self.target_kl > 0.0:
                raise L.AmenvError(f"target_kl must be positive (got {target_kl!r}); None switches the early stop off")
            if self.world > 1:
                raise L.AmenvError("target_kl with several ranks is not built: every rank would take the stop decision from its own shard's approx_kl and "
                                   "the ranks would disagree on it (no multi-GPU machine was available to test an agreed stop); train with target_kl=None")
            if use_graph:
                raise L.AmenvError("target_kl with use_graph=True is not built: the early stop sits between the loss and the optimiser step, inside "
                                   "what a captured graph replays as one piece; leave use_graph unset (target_kl runs the eager paths)")
            use_graph = False
        # two graphs around an eager all-reduce whenever there is a process group to talk to (tests force it with 1 rank)
        self.split = (self.world > 1) if split_graphs is None else bool(split_graphs)
        self.clip_range, self.ent_coef, self.vf_coef = float(clip_range), float(ent_coef), float(vf_coef)
        self.max_grad_norm, self.normalize_advantage = max_grad_norm, bool(normalize_advantage)
        dev = policy.flat_param.device
        capturable = all(g.get("capturable", False) for g in optimizer.param_groups) if hasattr(optimizer, "param_groups") else False
        self.use_graph = (dev.type == "cuda" and capturable) if use_graph is None else bool(use_graph)
        self.stats = torch.zeros(5, device=dev)          # policy loss, value loss, entropy loss, clip fraction, grad norm
        self._params = list(policy.parameters())         # in flat-buffer order (flatten_ walks parameters() the same way)
        assert self._params[0] is policy.log_std
        self._net_params = self._params[1:]
        # loss + its gradient in the HIP kernels (amenv_ppo_loss_grad) on the GPU; the torch expression is the host-side statement
        self.fused_loss = (dev.type == "cuda") if fused_loss is None else bool(fused_loss)
        self._fused_buf = None
        # the whole forward / loss / backward of both MLPs in ONE kernel on the fp32 matrix cores (amenv_ppo_mlp_step) where the policy
        # has the reference's architecture; the torch modules + fused loss otherwise
        ok = dev.type == "cuda" and getattr(policy, "net_arch", None) == (128, 64, 64) and (policy.obs_dim, policy.act_dim) in policy._FUSED_DIMS
        self.fused_mlp = ok if fused_mlp is None else (bool(fused_mlp) and ok)
        self._mlp_ws = None
        # clip + Adam in one launch on torch.optim.Adam's own state tensors (amenv_ppo_adam_step) where the optimiser is the plain Adam
        # on the flat buffer that `PPO` builds; anything else steps through torch
        self.fused_adam = self.fused_mlp and self._adam_is_plain(optimizer, policy)
        self._adam_hyper = self._adam_key = self._adam_ticket = None
        if self.fused_mlp and use_graph is None:
            self.use_graph = False                       # five launches per minibatch: nothing left for a graph to save
        self._static = None
        self._graphs = None
        self._eager_calls = 0
        # the device control block (amenv_ppo_ctl) of the HIP paths: the gate where the whole step is HIP, approx_kl and the running sums everywhere
        self.device_gate = self.target_kl is not None and self.fused_mlp and self.fused_adam
        self.device_rule = self.adaptive_lr is not None and self.fused_mlp and self.fused_adam   # the rule inside the fused Adam step
        self._lr_on_device = False                       # device_rule: an update has started, hyper6[0] is the device's until `readout`
        self._ctl = None
        if dev.type == "cuda" and (self.fused_loss or self.fused_mlp):
            if L.load().amenv_ppo_ctl_bytes() != C.sizeof(L.PpoCtl):
                raise L.AmenvError("amenv_ppo_ctl: the library's layout differs from this package's (rebuild libamenv.so)")
            self._ctl = torch.zeros(C.sizeof(L.PpoCtl) // 4, dtype=torch.int32, device=dev)
        k = L.PpoCtl.kl_last.offset // 4
        self.kl = torch.zeros(1, device=dev) if self._ctl is None else self._ctl.view(torch.float32)[k:k + 1]   # approx_kl of the last minibatch
        # host side of the gate (every path but the device gate): sums over the evaluated minibatches, counters, the stop
        self._acc = torch.zeros(6, device=dev)
        self.evaluated = self.applied = 0
        self.stopped = False
        self.arm()

    # -- training controls -------------------------------------------------------------------------
    def _ctl_ptr(self):
        return None if self._ctl is None else C.c_void_p(self._ctl.data_ptr())

    def arm(self):
        """Start an update: counters and sums to zero, the gate open (asynchronous: one tiny launch on the current stream)."""
        if self._ctl is not None:
            limit = 1.5 * self.target_kl if self.device_gate else 0.0
            rc = L.load().amenv_ppo_ctl_arm(self._ctl_ptr(), limit, C.c_void_p(torch.cuda.current_stream(self._ctl.device).cuda_stream))
            if rc != 0:
                raise L.AmenvError(f"amenv_ppo_ctl_arm failed ({rc})")
        self._acc.zero_()
        self.evaluated = self.applied = 0
        self.stopped = False
        self._lr_on_device = False

    def set_hyper(self, learning_rate=None, clip_range=None, clip_range_vf=None):
        changed = False
        if clip_range is not None and float(clip_range) != self.clip_range:
            self.clip_range, changed = float(clip_range), True
        if clip_range_vf is not None and float(clip_range_vf) != self.clip_range_vf:
            if self.clip_range_vf is None or not (float(clip_range_vf) > 0.0 and math.isfinite(float(clip_range_vf))):
                raise L.AmenvError("set_hyper: clip_range_vf changes a value clip that was built in (positive, finite); it does not switch one on")
            self.clip_range_vf, changed = float(clip_range_vf), True
        if learning_rate is not None:
            for g in self.optimizer.param_groups:
                if isinstance(g["lr"], torch.Tensor):
                    g["lr"].fill_(float(learning_rate))
                elif g["lr"] != float(learning_rate):
                    g["lr"] = float(learning_rate)
                    if self.fused_adam:                  # the fused Adam step reads lr from `hyper6` on the device, inside a replayed graph too
                        if self._adam_hyper is not None:
                            self._adam_upload_hyper()
                    else:
                        changed = True                   # torch's Adam took the Python float into the capture
        if changed and self._graphs is not None:         # baked into a capture: capture again at the next full minibatch
            self._graphs = self._static = None

    # -- the arithmetic (shared by the eager and the captured path) --------------------------------
    def _old_values(self, old_values):
        if (self.clip_range_vf is None) != (old_values is None):
            raise L.AmenvError("old_values go with clip_range_vf: the clipped value loss needs the rollout's values, and nothing else reads them")
        return old_values

    def _forward_backward(self, obs, actions, old_logp, adv, ret, old_values=None):
        self._old_values(old_values)
        if self.fused_mlp:
            return self._forward_backward_mlp(obs, actions, old_logp, adv, ret, None, old_values)
        if self.fused_loss:
            return self._forward_backward_fused(obs, actions, old_logp, adv, ret, old_values)
        if self.normalize_advantage and adv.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        values, logp, entropy = self.policy.evaluate_actions(obs, actions)
        log_ratio = logp - old_logp
        ratio = torch.exp(log_ratio)
        c = self.clip_range
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)).mean()
        if old_values is not None:                       # SB3: values_pred = old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf)
            values = old_values + torch.clamp(values - old_values, -self.clip_range_vf, self.clip_range_vf)
        vl = torch.nn.functional.mse_loss(ret, values)
        el = -entropy.mean()
        # gradients straight into the flat buffer with ONE concatenation (autograd's per-parameter accumulate-into-.grad would
        # be 17 tiny read-modify-write kernels plus a zero fill per minibatch)
        grads = torch.autograd.grad(pl + self.ent_coef * el + self.vf_coef * vl, self._params)
        torch.cat([g.reshape(-1) for g in grads], out=self.policy.flat_grad)
        with torch.no_grad():
            self.stats[0], self.stats[1], self.stats[2] = pl.detach(), vl.detach(), el.detach()
            self.stats[3] = ((ratio.detach() - 1.0).abs() > c).float().mean()
            self.kl[0] = ((ratio.detach() - 1.0) - log_ratio.detach()).mean()         # SB3's approx_kl

    def _forward_backward_fused(self, obs, actions, old_logp, adv, ret, old_values=None):
        """Same loss, with everything between the network outputs and the backward pass in the HIP kernels of
        `amenv_ppo_loss_grad` (3 launches for ~60): autograd only walks the two MLPs, seeded with d L / d mean and d L / d value."""
        pol = self.policy
        mean, values = pol.actor(obs), pol.critic(obs)
        n, a = mean.shape
        if self._fused_buf is None or self._fused_buf[0].shape[0] != n:
            f = dict(dtype=torch.float32, device=mean.device)
            self._fused_buf = (torch.empty(n, a, **f), torch.empty(n, **f), torch.empty(a, **f),
                               torch.empty(L.load().amenv_ppo_workspace_bytes() // 8, dtype=torch.float64, device=mean.device))
        d_mean, d_value, d_log_std, ws = self._fused_buf
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        m, v = mean.detach().contiguous(), values.detach().contiguous()
        args = (p(m), p(v), p(pol.log_std.detach()), p(actions), p(old_logp), p(adv), p(ret), n, a, self.clip_range, self.ent_coef, self.vf_coef,
                1 if self.normalize_advantage else 0, p(d_mean), p(d_value), p(d_log_std), p(self.stats), p(ws), self._ctl_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(mean.device).cuda_stream)
        if old_values is None:
            rc = L.load().amenv_ppo_loss_grad_ctl(*args, stream)
        else:
            rc = L.load().amenv_ppo_loss_grad_vclip(*args, p(old_values.contiguous()), self.clip_range_vf, stream)
        if rc != 0:
            raise L.AmenvError(f"amenv_ppo_loss_grad failed ({rc})")
        grads = torch.autograd.grad([mean, values], self._net_params, grad_outputs=[d_mean, d_value])
        torch.cat([d_log_std] + [g.reshape(-1) for g in grads], out=pol.flat_grad)     # log_std is the first parameter

    @staticmethod
    def _adam_is_plain(opt, policy):
        if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1 or len(opt.param_groups[0]["params"]) != 1:
            return False
        g = opt.param_groups[0]
        p = g["params"][0]
        return (p.data_ptr() == policy.flat_param.data_ptr() and p.numel() == policy.flat_param.numel() and g.get("capturable", False)
                and not g.get("amsgrad") and not g.get("maximize") and g.get("weight_decay", 0) == 0 and not g.get("decoupled_weight_decay", False)
                and not isinstance(g["lr"], torch.Tensor))

    def _forward_backward_mlp(self, obs, actions, old_logp, adv, ret, index=None, old_values=None):
        """Forward, SB3's loss, backward and every weight gradient in ONE kernel (csrc/amenv_mlp_train.hpp): the gradient lands in the flat
        buffer, the four reported scalars in `stats`.  fp32 throughout (v_mfma_f32_32x32x2_f32), autograd is not involved.  With `index`
        (int64 [n]) the minibatch is rows `index` of the given tensors, gathered inside the kernel."""
        pol = self.policy
        if self._mlp_ws is None:
            self._mlp_ws = torch.empty(L.load().amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device=obs.device)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        obs, actions = obs.contiguous(), actions.contiguous()
        n = obs.shape[0] if index is None else index.shape[0]
        args = (p(pol.flat_param.detach()), pol.obs_dim, pol.act_dim, p(obs), p(actions), p(old_logp), p(adv), p(ret),
                None if index is None else p(index), n, self.clip_range, self.ent_coef, self.vf_coef, 1 if self.normalize_advantage else 0, p(pol.flat_grad), p(self.stats),
                p(self._mlp_ws), self._ctl_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        if self._old_values(old_values) is None:
            rc = L.load().amenv_ppo_mlp_step_ctl(*args, stream)
        else:
            rc = L.load().amenv_ppo_mlp_step_vclip(*args, p(old_values.contiguous()), self.clip_range_vf, stream)
        if rc != 0:
            raise L.AmenvError(f"amenv_ppo_mlp_step failed ({rc})")

    def _exchange(self):
        if self.dist is not None and (self.world > 1 or self.split):
            self.dist.all_reduce(self.policy.flat_grad)
            if self.world > 1 and not self.fused_adam:   # (the fused Adam step folds 1 / world into its gradient scale)
                self.policy.flat_grad.div_(self.world)

    def _apply_fused(self):
        """Clip + Adam as one launch on the optimiser's own state (so `optimizer.state_dict()` and checkpoints stay torch's)."""
        opt, pol = self.optimizer, self.policy
        g = opt.param_groups[0]
        leaf = g["params"][0]
        st = opt.state[leaf]
        if not st:                                       # torch.optim.Adam creates its state on the first step
            st["step"] = torch.zeros((), dtype=torch.float32, device=leaf.device)
            st["exp_avg"] = torch.zeros_like(pol.flat_param)
            st["exp_avg_sq"] = torch.zeros_like(pol.flat_param)
        self._adam_upload_hyper()
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        args = (p(pol.flat_param.detach()), p(pol.flat_grad), p(st["exp_avg"]), p(st["exp_avg_sq"]), p(st["step"]), pol.flat_param.numel(),
                p(self._adam_hyper), C.c_void_p(self.stats.data_ptr() + 16), p(self._adam_ticket), self._ctl_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(leaf.device).cuda_stream)
        if self.device_rule:                             # the rule inside the launch; from here to `readout` hyper6[0] is the device's
            rc = L.load().amenv_ppo_adam_step_adapt(*args, C.byref(self.adaptive_lr.struct()), stream)
            self._lr_on_device = True
        else:
            rc = L.load().amenv_ppo_adam_step_ctl(*args, stream)
        if rc != 0:
            raise L.AmenvError(f"amenv_ppo_adam_step failed ({rc})")

    def _adam_upload_hyper(self):
        """hyper6 of the fused Adam step on the device, re-uploaded when a value changed (a host-to-device copy: `_capture` calls this
        BEFORE it starts capturing, a copy from pageable memory is not allowed inside a capture)."""
        g = self.optimizer.param_groups[0]
        key = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
               float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0, 1.0 / self.world)
        if self._lr_on_device and self._adam_key is not None:
            # adaptive_lr on the device, an update under way: the host's copy of the rate is stale and hyper6[0] is not the host's to write
            if key[1:] != self._adam_key[1:]:
                self._adam_hyper[1:].copy_(torch.tensor(key[1:], dtype=torch.float32))
                self._adam_key = self._adam_key[:1] + key[1:]
            return
        if key != self._adam_key:
            dev = g["params"][0].device
            if self._adam_hyper is None:
                self._adam_hyper = torch.empty(6, dtype=torch.float32, device=dev)
                self._adam_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            self._adam_hyper.copy_(torch.tensor(key, dtype=torch.float32))
            self._adam_key = key

    def _apply(self):
        if self.fused_adam:
            return self._apply_fused()
        g = self.policy.flat_grad
        gn = g.norm(2)
        if self.max_grad_norm is not None:
            g.mul_(torch.clamp(self.max_grad_norm / (gn + 1e-6), max=1.0))
        self.optimizer.step()
        self.stats[4] = gn

    def _host_gate(self):
        """SB3's check where the step is not all HIP: between the loss and the optimiser step, one host synchronisation.  True: stop."""
        if self.target_kl is None or self.device_gate:
            return False
        self._acc[:4] += self.stats[:4]
        self._acc[5:] += self.kl
        self.evaluated += 1
        if float(self.kl) > 1.5 * self.target_kl:
            self.stopped = True
        return self.stopped

    def _applied(self):
        if self.target_kl is not None and not self.device_gate:
            self._acc[4] += self.stats[4]
            self.applied += 1

    def _host_rule(self):
        """`KlAdaptiveLr.step` where the step is not all HIP: after the loss (and the stop test), before the optimiser step; one host
        synchronisation, as the host `target_kl` check takes.  (Never beside the device gate: gate and rule are on the device together.)"""
        if self.adaptive_lr is None or self.device_rule:
            return
        for g in self.optimizer.param_groups:
            lr = g["lr"]
            new = float(self.adaptive_lr.step(float(lr), float(self.kl)))
            if isinstance(lr, torch.Tensor):
                lr.fill_(new)
            else:
                g["lr"] = new

    def _eager(self, *mb):
        if self.stopped:
            return
        self._forward_backward(*mb)
        if self._host_gate():
            return
        self._host_rule()
        self._exchange()
        self._apply()
        self._applied()

    def indexed(self, obs, actions, old_logp, adv, ret, index, old_values=None):
        """One minibatch step on rows `index` of the whole-rollout tensors (fused path only): no gathered copies, no graph."""
        if self.stopped:
            return
        self._forward_backward_mlp(obs, actions, old_logp, adv, ret, index, old_values)
        if self._host_gate():
            return
        self._host_rule()
        self._exchange()
        self._apply()
        self._applied()

    def readout(self, total, n_batches, extra=None):
        """The record of an update from ONE device-to-host transfer: `total` (the last epoch's sums of `stats` and `kl` over `n_batches`
        minibatches), the control block and `extra` (name -> 0-dim device tensor).  Without target_kl: last-epoch means, the meaning the
        five loss keys always had.  With it: means over every minibatch that was EVALUATED in the whole update (the gradient norm: over
        the steps applied), as SB3 logs them -- the last epoch may not have run."""
        extra = extra or {}
        parts = [total.to(torch.float32).view(torch.int32), self._acc.view(torch.int32)]   # (as raw words: the block's counters are integers)
        if self._ctl is not None:
            parts.append(self._ctl)
        lr_back = self.device_rule and self._adam_hyper is not None
        if lr_back:                                      # the learning rate the device rule arrived at, with the same transfer
            parts.append(self._adam_hyper[:1].view(torch.int32))
        parts += [v.detach().reshape(1).to(torch.float32).view(torch.int32) for v in extra.values()]
        host = torch.cat(parts).cpu().numpy().view(np.float32)
        tot, acc = host[:6].astype(np.float64), host[6:12].astype(np.float64)
        k = 12
        evaluated, applied, stopped = self.evaluated, self.applied, self.stopped
        if self._ctl is not None:
            c = L.PpoCtl.from_buffer_copy(host[k:k + self._ctl.numel()].tobytes())
            k += self._ctl.numel()
            if self.device_gate:
                acc = np.array([c.sum[0], c.sum[1], c.sum[2], c.sum[3], c.sum[4], c.kl_sum], dtype=np.float64)
                evaluated, applied, stopped = int(c.evaluated), int(c.applied), bool(c.stop)
        if lr_back:                                      # back to the host: param_groups and the upload key agree with hyper6[0] again
            lr = float(host[k])
            k += 1
            self.optimizer.param_groups[0]["lr"] = lr
            if self._adam_key is not None:
                self._adam_key = (lr,) + self._adam_key[1:]
            self._lr_on_device = False
        if self.target_kl is None:
            s = tot / max(n_batches, 1)
            n_updates, stopped = None, False
        else:
            s = acc / max(evaluated, 1)
            s[4] = acc[4] / max(applied, 1)
            n_updates = applied
        rec = dict(policy_loss=float(s[0]), value_loss=float(s[1]), entropy_loss=float(s[2]), clip_fraction=float(s[3]), grad_norm=float(s[4]),
                   approx_kl=float(s[5]), kl_early_stop=int(stopped))
        for name, v in zip(extra, host[k:]):
            rec[name] = float(v)
        return rec, n_updates

    # -- graph capture --------------------------------------------------------------------------
    def _capture(self, mb):
        self._static = tuple(torch.empty_like(t) for t in mb)
        for s, t in zip(self._static, mb):
            s.copy_(t)
        if self.fused_adam:
            self._adam_upload_hyper()
        torch.cuda.synchronize()
        g1 = torch.cuda.CUDAGraph()
        if not self.split:
            with torch.cuda.graph(g1):
                self._forward_backward(*self._static)
                self._apply()
            self._graphs = (g1, None)
        else:
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1):
                self._forward_backward(*self._static)
            with torch.cuda.graph(g2, pool=g1.pool()):
                self._apply()
            self._graphs = (g1, g2)

    def __call__(self, obs, actions, old_logp, adv, ret, old_values=None):
        mb = (obs, actions, old_logp, adv, ret) + (() if self._old_values(old_values) is None else (old_values,))
        full = self._static is None or obs.shape[0] == self._static[0].shape[0]
        if not self.use_graph or not full:
            return self._eager(*mb)
        if self._graphs is None:
            if self._eager_calls < 3:                    # warm-up: real updates, run eagerly (library handles, autotuning)
                self._eager_calls += 1
                return self._eager(*mb)
            try:
                self._capture(mb)                        # records only; the replay below performs this minibatch
            except Exception as e:  # noqa: BLE001 - capture is an optimisation: report and keep training eagerly
                import warnings
                warnings.warn(f"PPO minibatch graph capture failed ({type(e).__name__}: {e}); continuing without graphs")
                self.use_graph, self._static, self._graphs = False, None, None
                return self._eager(*mb)
        else:
            for s, t in zip(self._static, mb):
                s.copy_(t)
        g1, g2 = self._graphs
        g1.replay()
        if g2 is not None:
            self._exchange()
            g2.replay()


def ppo_update(policy, optimizer, obs, actions, old_logp, advantages, returns, *, batch_size, n_epochs, clip_range=0.2,
               ent_coef=5e-4, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True, generator=None, dist=None, step=None, target_kl=None,
               extra=None, adaptive_lr=None, clip_range_vf=None, old_values=None):
    """SB3 `PPO.train()` on flattened rollout tensors (obs [n, D], actions [n, A], the rest [n]).  Device-agnostic torch;
    with `dist` (an initialised torch.distributed, RCCL on GPUs) every minibatch gradient is averaged over ranks with ONE
    all-reduce of the policy's flat gradient buffer.  `step`: a persistent `MinibatchStep` (keeps its captured graphs
    between calls; its own `target_kl` holds).  Returns policy_loss, value_loss, entropy_loss, clip_fraction, grad_norm and approx_kl as
    means of the last epoch (one host sync), `n_updates` (optimiser steps applied by this call) and `kl_early_stop` (0 / 1).

    `target_kl`: SB3's early stop (see `MinibatchStep`).  On the all-HIP path the loop below keeps launching and the device gate makes
    the remaining launches no-ops: still one host sync per update.  On the other paths the host checks every minibatch and breaks.  With
    it the six scalars are means over every evaluated minibatch of the update.  `extra`: name -> 0-dim device tensor, or a callable
    returning one that is evaluated after the last minibatch; fetched with the same transfer and returned under its name.

    `adaptive_lr` (a `KlAdaptiveLr`): the learning rate follows every minibatch's approx_kl (see `MinibatchStep`); `optimizer.param_groups[0]
    ["lr"]` holds the rate the update arrived at when this returns.  `clip_range_vf` + `old_values` [n]: SB3's clipped value loss against
    the rollout's values.  As with `target_kl`, a `step` that is passed in holds its own settings."""
    n = obs.shape[0]
    if step is None:
        step = MinibatchStep(policy, optimizer, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                             normalize_advantage=normalize_advantage, dist=dist, use_graph=False, target_kl=target_kl, adaptive_lr=adaptive_lr,
                             clip_range_vf=clip_range_vf)
    elif target_kl is not None and step.target_kl != float(target_kl):
        raise L.AmenvError(f"ppo_update: target_kl={target_kl!r} but the MinibatchStep given was built with target_kl={step.target_kl!r}")
    elif adaptive_lr is not None and step.adaptive_lr != adaptive_lr:
        raise L.AmenvError(f"ppo_update: adaptive_lr={adaptive_lr!r} but the MinibatchStep given was built with adaptive_lr={step.adaptive_lr!r}")
    elif clip_range_vf is not None and step.clip_range_vf != float(clip_range_vf):
        raise L.AmenvError(f"ppo_update: clip_range_vf={clip_range_vf!r} but the MinibatchStep given was built with clip_range_vf={step.clip_range_vf!r}")
    step._old_values(old_values)
    vclip = () if old_values is None else (old_values,)
    step.arm()
    total = torch.zeros(6, device=obs.device)
    n_batches = 0
    for epoch in range(n_epochs):
        if step.stopped:                                 # (host gate only: the device gate never tells the host before the end)
            break
        # one shuffle of the whole buffer per epoch (5 gathers), then every minibatch is a contiguous slice
        perm = torch.randperm(n, device=obs.device, generator=generator)
        indexed = step.fused_mlp and not step.use_graph
        if not indexed:
            obs_s, act_s, olp_s, adv_s, ret_s = obs[perm], actions[perm], old_logp[perm], advantages[perm], returns[perm]
            val_s = None if old_values is None else old_values[perm]
        for start in range(0, n, batch_size):
            sl = slice(start, min(start + batch_size, n))
            if indexed:                                  # the kernel reads rows perm[sl] itself
                step.indexed(obs, actions, old_logp, advantages, returns, perm[sl], *vclip)
            else:
                step(obs_s[sl], act_s[sl], olp_s[sl], adv_s[sl], ret_s[sl], *(() if val_s is None else (val_s[sl],)))
            if step.stopped:
                break
            if epoch == n_epochs - 1:   # losses are reported for the last epoch only (no host sync inside the loop)
                total[:5] += step.stats
                total[5:] += step.kl
                n_batches += 1
    extra = {k: (v() if callable(v) else v) for k, v in (extra or {}).items()}
    rec, n_updates = step.readout(total, n_batches, extra)
    rec["n_updates"] = n_epochs * ((n + batch_size - 1) // batch_size) if n_updates is None else n_updates
    return rec


class PPO:
    """The reference's training loop (`model = PPO(...); model.learn(...)`, v2/rl_train.py:38-56) with the rollout resident
    on the GPU.  `env` is a `GpuWaypointEnv` (auto-reset on); defaults are the reference's hyper-parameters -- with thousands
    of envs scale `n_steps` down and `batch_size` up.

    `reward_normalizer` (a `RewardNormalizer` over the env's num_envs; None = raw rewards, the reference's set-up): what an SB3 loop over
    `VecNormalize(norm_reward=True)` feeds its buffer.  On both rollout paths the [n_steps, N] pass runs ONCE after the rollout on the raw
    `buffer.rewards` / `buffer.dones` (normalised rewards never feed back into the rollout, so this equals the per-step wrapper bit for
    bit), THEN the time-limit bootstrap gamma * V(terminal_observation) is added, then GAE -- SB3's order, where the bootstrap is added to
    the already normalised reward.  Its discount is the normaliser's own `gamma` (SB3's VecNormalize default .99, not PPO's).  With `dist`
    the return statistics are per rank, as the observation normaliser's are: every rank scales with the statistics of its own shard.
    `env.stats()` and the logged `ep_rew_mean` stay raw.

    `adaptive_lr` (a `KlAdaptiveLr`): `learning_rate` is the starting value and every minibatch's approx_kl moves it -- inside the
    fused Adam step on the GPU's default update path, on the host elsewhere (`MinibatchStep`); the record's `learning_rate` is the value
    after the update; a `learning_rate` schedule beside it, several ranks and `use_graph=True` raise.  `clip_range_vf` (a float or a
    schedule of progress_remaining; None = off): SB3's clipped value loss against `buffer.values`."""

    def __init__(self, env, policy=None, learning_rate=2e-4, n_steps=2048, batch_size=128, n_epochs=12, gamma=0.995,
                 gae_lambda=0.9, clip_range=0.2, ent_coef=5e-4, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True,
                 net_arch=(128, 64, 64), seed=0, obs_normalizer=None, bootstrap_truncated=True, dist=None, use_graph=None, fused_rollout=False, fused_mlp=None, fused_rollout_fp32_stats=True,
                 reward_normalizer=None, target_kl=None, adaptive_lr=None, clip_range_vf=None):
        if env.state_dtype != torch.float32:
            raise L.AmenvError("PPO needs the fp32 environment")
        self.env, self.dist = env, dist
        self.world = dist.get_world_size() if dist is not None else 1
        self.target_kl = None if target_kl is None else float(target_kl)
        if self.target_kl is not None and self.world > 1:
            raise L.AmenvError("target_kl with several ranks is not built: every rank would take the stop decision from its own shard's approx_kl and "
                               "the ranks would disagree on it (no multi-GPU machine was available to test an agreed stop); train with target_kl=None")
        self.adaptive_lr = adaptive_lr
        if adaptive_lr is not None:
            if not isinstance(adaptive_lr, KlAdaptiveLr):
                raise L.AmenvError(f"adaptive_lr must be a KlAdaptiveLr or None (got {type(adaptive_lr).__name__})")
            if callable(learning_rate):
                raise L.AmenvError("a learning_rate schedule together with adaptive_lr: two masters for one number; pass the starting value as a float")
            if self.world > 1:
                raise L.AmenvError("adaptive_lr with several ranks is not built: every rank would move its learning rate by its own shard's approx_kl and "
                                   "the ranks would step with different rates; train with adaptive_lr=None")
        # SB3's Schedule: a float, or a callable of progress_remaining (1 at the start of `learn`, towards 0 at its end)
        self._lr_fn = learning_rate if callable(learning_rate) else None
        self._clip_fn = clip_range if callable(clip_range) else None
        self._clip_vf_fn = clip_range_vf if callable(clip_range_vf) else None
        if self._clip_vf_fn is not None:
            clip_range_vf = float(self._clip_vf_fn(1.0))
        self.clip_range_vf = None if clip_range_vf is None else float(clip_range_vf)
        self._progress = 1.0
        if self._lr_fn is not None:
            learning_rate = float(self._lr_fn(1.0))
        if self._clip_fn is not None:
            clip_range = float(self._clip_fn(1.0))
        self.device = env.device
        self.n_steps, self.batch_size, self.n_epochs = int(n_steps), int(batch_size), int(n_epochs)
        self.gamma, self.gae_lambda, self.clip_range = float(gamma), float(gae_lambda), float(clip_range)
        self.ent_coef, self.vf_coef, self.max_grad_norm = float(ent_coef), float(vf_coef), max_grad_norm
        self.normalize_advantage, self.bootstrap_truncated = bool(normalize_advantage), bool(bootstrap_truncated)
        self.seed = int(seed)
        torch.manual_seed(self.seed)   # identical initial weights on every rank (also broadcast below)
        if policy is None:
            policy = ActorCritic(env.obs_dim, env.act_dim, net_arch)
        if policy.obs_dim != env.obs_dim or policy.act_dim != env.act_dim:
            raise L.AmenvError(f"policy is {policy.obs_dim}->{policy.act_dim}, env is {env.obs_dim}->{env.act_dim}")
        self.policy = policy.to(self.device).flatten_()
        if self.world > 1:
            dist.broadcast(self.policy.flat_param, src=0)
        self._leaf = self.policy.flat_param.requires_grad_(True)
        self._leaf.grad = self.policy.flat_grad
        self.optimizer = torch.optim.Adam([self._leaf], lr=learning_rate, eps=1e-5, capturable=self.device.type == "cuda")
        self._step = MinibatchStep(self.policy, self.optimizer, clip_range=self.clip_range, ent_coef=self.ent_coef, vf_coef=self.vf_coef,
                                   max_grad_norm=self.max_grad_norm, normalize_advantage=self.normalize_advantage,
                                   dist=dist if self.world > 1 else None, use_graph=use_graph, fused_mlp=fused_mlp, target_kl=self.target_kl,
                                   adaptive_lr=adaptive_lr, clip_range_vf=self.clip_range_vf)
        self.n_updates = 0   # optimiser steps applied so far (SB3's `_n_updates` counts epochs; with an early stop inside an epoch steps are the honest unit)
        self.obs_normalizer = obs_normalizer
        self.reward_normalizer = reward_normalizer
        if reward_normalizer is not None and int(reward_normalizer.num_envs) != int(env.num_envs):
            raise L.AmenvError(f"reward_normalizer holds {reward_normalizer.num_envs} envs, the env has {env.num_envs}")
        self._boot = None   # [n_steps, N] V(terminal_observation) at the truncated entries of the step-by-step rollout, added after the reward pass
        self.buffer =RolloutBuffer(self.n_steps, env.num_envs, env.obs_dim, env.act_dim, self.device)
        self._clipped = torch.zeros(env.num_envs, env.act_dim, dtype=torch.float32, device=self.device)
        self._raw_obs = torch.zeros(env.num_envs, env.obs_dim, dtype=torch.float32, device=self.device) if obs_normalizer else None
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed * 1000003 + int(getattr(env.cfg, "env_id_offset", 0)))
        self._draw = 0
        self._started = False
        # opt-in: the whole rollout (policy MLPs on the bf16 matrix cores, sampling, clip, env step) in ONE launch -- amenv_rollout_policy
        self.fused_rollout = bool(fused_rollout)
        self.fused_rollout_fp32_stats = bool(fused_rollout_fp32_stats)   # fused rollout: store the fp32 policy's log-probs / values (SB3's buffer semantics)
        if self.fused_rollout and obs_normalizer is not None and getattr(env, "action_history", None) is not None:
            raise L.AmenvError("fused_rollout with an observation normaliser is not built with the action history (amenv_rollout_policy_norm refuses it): "
                               "use the step-by-step rollout (fused_rollout=False) with the normaliser, or fused_rollout without one")
        if self.fused_rollout and obs_normalizer is not None and int(env.cfg.vehicle.n_joints) != 0:
            raise L.AmenvError("fused_rollout with an observation normaliser is built for the rigid vehicles (amenv_rollout_policy_norm); "
                               "arm vehicles: fused_rollout without a normaliser, or the step-by-step rollout")
        self._term_obs = self._info = None
        self.num_timesteps = 0
        self.log = []

    # ---- rollout --------------------------------------------------------------------------------
    def _first_obs(self):
        obs = self.env.reset()
        if self.obs_normalizer is not None:
            self.obs_normalizer.update(obs)
            self.obs_normalizer.normalize(obs, out=self.buffer.obs[0])
        else:
            self.buffer.obs[0].copy_(obs)
        self._started = True

    @torch.no_grad()
    def collect_rollouts(self):
        """SB3 `OnPolicyAlgorithm.collect_rollouts`: n_steps steps of every env into the buffer, then GAE."""
        b, env, pol = self.buffer, self.env, self.policy
        if self.fused_rollout:
            return self._collect_rollouts_fused()
        if not self._started:
            self._first_obs()
        else:
            b.obs[0].copy_(b.obs[self.n_steps])
        gid0 = int(env.cfg.env_id_offset)
        rnorm = self.reward_normalizer
        if rnorm is not None and self.bootstrap_truncated and self._boot is None:
            self._boot = torch.zeros(self.n_steps, env.num_envs, dtype=torch.float32, device=self.device)
        for t in range(self.n_steps):
            obs_t = b.obs[t]
            mean_t, value_t = pol.actor_critic(obs_t)
            b.values[t].copy_(value_t)
            gaussian_act(mean_t, pol.log_std.data, pol.action_low, pol.action_high, b.actions[t], self._clipped, b.logp[t],
                         self.seed, self._draw, gid0)
            self._draw += 1
            if self.obs_normalizer is None:
                env.step_into(self._clipped, b.obs[t + 1], b.rewards[t], b.dones[t])
                term_obs = env.terminal_obs
            else:   # VecNormalize(norm_obs=True): statistics from the raw observations, the learner sees normalised ones
                env.step_into(self._clipped, self._raw_obs, b.rewards[t], b.dones[t])
                self.obs_normalizer.update(self._raw_obs)
                self.obs_normalizer.normalize(self._raw_obs, out=b.obs[t + 1])
                term_obs = self.obs_normalizer.normalize(env.terminal_obs) if self.bootstrap_truncated else None
            if self.bootstrap_truncated:
                # SB3: reward += gamma * V(terminal_observation) where the episode was cut by the time limit only
                trunc = ((env.info_bits & (L.INFO_TERMINATED | L.INFO_TRUNCATED)) == L.INFO_TRUNCATED) & (b.dones[t] != 0)
                if rnorm is None:
                    b.rewards[t].addcmul_(pol.critic(term_obs), trunc.to(torch.float32), value=self.gamma)
                else:   # deferred: the bootstrap joins the NORMALISED reward (SB3's order), so the rewards stay raw until the pass below
                    torch.mul(pol.critic(term_obs), trunc.to(torch.float32), out=self._boot[t])
        if rnorm is not None:
            rnorm.normalize(b.rewards, b.dones, out=b.rewards)
            if self.bootstrap_truncated:
                b.rewards.add_(self._boot, alpha=self.gamma)
        b.last_values.copy_(pol.critic(b.obs[self.n_steps]))
        compute_gae(b, self.gamma, self.gae_lambda)
        self.num_timesteps += self.n_steps * env.num_envs * self.world
        return b

    def _collect_rollouts_fused(self):
        """collect_rollouts as ONE kernel launch (csrc/amenv_team_policy.hpp): n_steps x (actor / critic forward in bf16 on the matrix
        cores -> Gaussian sample -> clip -> env step) with state, constants and weights in registers; the buffer rows are written by the
        kernel.  What stays on the host side of the launch: the time-limit bootstrap reward += gamma V(terminal_observation) (one critic
        call over the truncated entries), V of the last observation, GAE.  The rollout policy is the bf16 rounding of the fp32 policy the
        update differentiates (means differ by ~1e-2 of their scale): PPO's clipped ratio absorbs that; log-probs are those of the
        samples under the means the kernel used.

        With an observation normaliser (rigid vehicles) it runs inside the launch (amenv_rollout_policy_norm): the statistics are FROZEN for
        the rollout -- every buffer row, the policy's input and the terminal rows are normalised with the statistics at its start -- and
        merge the raw rows 1..n_steps once at its end, where SB3's VecNormalize updates them before every step.  The policy and the learner
        see the same rows; the step-by-step path keeps SB3's order."""
        b, env, pol, T = self.buffer, self.env, self.policy, self.n_steps
        norm = self.obs_normalizer
        if not self._started:
            obs = env.reset()
            if norm is not None:   # as _first_obs: the reset rows count once, row 0 of the first launch is not counted again
                norm.update(obs)
            self._started = True
        if self._term_obs is None:
            self._term_obs = torch.zeros(T, env.num_envs, env.obs_dim, dtype=torch.float32, device=self.device)
            self._info = torch.zeros(T, env.num_envs, dtype=torch.int32, device=self.device)
        env.rollout_policy(pol.flat_param, T, self.seed, self._draw, b.obs, b.actions, b.logp, b.values, b.rewards, b.dones, self._info,
                           self._term_obs if self.bootstrap_truncated else None, obs_normalizer=norm)
        self._draw += T
        if self.fused_rollout_fp32_stats:
            # SB3's buffer holds log pi(a|s) and V(s) of the policy the update differentiates: re-evaluate the T*N rows with the fp32 policy (the
            # fused forward kernel: one launch) so that the first epoch's ratio is exactly 1 and the value targets are the fp32 critic's; the
            # samples themselves stay those of the bf16 behaviour policy (its means are ~1e-2 of their scale away)
            flat_obs = b.obs[:T].reshape(T * env.num_envs, env.obs_dim)
            mean, value = pol.actor_critic(flat_obs)
            ls = pol.log_std.data
            zz = (b.actions.reshape(T * env.num_envs, -1) - mean) * torch.exp(-ls)
            b.logp.copy_((-0.5 * zz * zz - ls - 0.918938533204672742).sum(1).reshape(T, env.num_envs))
            b.values.copy_(value.reshape(T, env.num_envs))
        if self.reward_normalizer is not None:   # the kernel wrote raw rewards; the bootstrap below joins the normalised ones (SB3's order)
            self.reward_normalizer.normalize(b.rewards, b.dones, out=b.rewards)
        if self.bootstrap_truncated:
            trunc = ((self._info & (L.INFO_TERMINATED | L.INFO_TRUNCATED)) == L.INFO_TRUNCATED) & (b.dones != 0)
            idx = trunc.reshape(-1).nonzero().reshape(-1)
            if idx.numel():
                v = pol.critic(self._term_obs.reshape(-1, env.obs_dim).index_select(0, idx))
                b.rewards.reshape(-1).index_add_(0, idx, self.gamma * v)
        b.last_values.copy_(pol.critic(b.obs[T]))
        compute_gae(b, self.gamma, self.gae_lambda)
        self.num_timesteps += T * env.num_envs * self.world
        return b

    # ---- update ---------------------------------------------------------------------------------
    @property
    def learning_rate(self):
        return float(self.optimizer.param_groups[0]["lr"])

    def train(self):
        """SB3 `PPO.train`: n_epochs passes over the buffer in shuffled minibatches, left early once approx_kl > 1.5 target_kl.

        Schedules (`learning_rate` / `clip_range` given as callables of progress_remaining) are evaluated here, once per call, at the
        progress `learn` set (1 outside `learn`), and take effect on every update path: the fused Adam step re-uploads its
        hyper-parameters, the torch optimiser reads its `param_groups`, and captured graphs -- which bake both values in -- are dropped
        and captured again when either changed (`MinibatchStep.set_hyper`).  Plain floats are left alone (a resumed checkpoint's
        learning rate stays).  The record adds to the losses: approx_kl, explained_variance (SB3's, over the buffer as stored before the
        update; 0.0 where the returns are constant), std (mean of exp(log_std) after the update), n_updates (cumulative optimiser steps),
        learning_rate, clip_range, kl_early_stop.  All of it comes with the update's one device-to-host transfer."""
        b, T = self.buffer, self.n_steps
        n = T * b.n_envs
        self._step.set_hyper(None if self._lr_fn is None else float(self._lr_fn(self._progress)),
                             None if self._clip_fn is None else float(self._clip_fn(self._progress)),
                             None if self._clip_vf_fn is None else float(self._clip_vf_fn(self._progress)))
        self.clip_range, self.clip_range_vf = self._step.clip_range, self._step.clip_range_vf
        rec = ppo_update(self.policy, self.optimizer, b.obs[:T].reshape(n, -1), b.actions.reshape(n, -1), b.logp.reshape(n),
                         b.advantages.reshape(n), b.returns.reshape(n), batch_size=self.batch_size, n_epochs=self.n_epochs,
                         generator=self._gen, step=self._step, old_values=None if self.clip_range_vf is None else b.values.reshape(n),
                         extra=dict(explained_variance=explained_variance(b.values, b.returns), std=lambda: self.policy.log_std.detach().exp().mean()))
        self.n_updates += int(rec["n_updates"])
        rec.update(n_updates=self.n_updates, learning_rate=self.learning_rate, clip_range=self.clip_range)
        return rec

    def _evaluate(self, eval_env, n_eval_episodes, deterministic):
        """One fused evaluation for `learn`: (mean, std, info).  Touches neither `_gen` nor `_draw` (a stochastic evaluation draws under its own
        key, the eval env's seed) nor the normaliser's statistics (used frozen)."""
        return _evaluate_fused(self, eval_env, n_eval_episodes, deterministic, None, seed=int(eval_env.cfg.seed), draw0=0)

    def learn(self, total_timesteps, log_fn=None, save_freq=None, save_path=None, name_prefix="ppo_model", eval_env=None, eval_freq=None,
              n_eval_episodes=None, eval_deterministic=True, best_model_save_path=None):
        """`model.learn(total_timesteps, callback=CheckpointCallback(save_freq, save_path, name_prefix))` (v2/rl_train.py:14-18,56):
        alternate rollouts and updates until the whole job has taken `total_timesteps` env steps.  Per iteration one record: losses +
        the Monitor episode statistics of the rollout.  `save_freq` counts env steps of the whole job (SB3 counts `VecEnv.step`
        calls: the reference's 12,500 calls x 8 envs = 100,000 steps); rank 0 writes `<save_path>/<name_prefix>_<steps>_steps.zip`
        at the first iteration boundary at or past every multiple.

        `eval_env` + `eval_freq` (SB3's `EvalCallback(eval_env, eval_freq=..., n_eval_episodes=..., deterministic=...,
        best_model_save_path=...)`): at the first iteration boundary at or past every multiple of `eval_freq` env steps (the `save_freq` rule)
        the policy is evaluated on `eval_env` -- a SEPARATE `GpuWaypointEnv` (the training env is refused: evaluation would cut its
        episodes) -- in one launch (`evaluate_policy(fused=True)`: the bf16 behaviour policy, the normaliser frozen), `n_eval_episodes`
        episodes (default: one per eval env).  That iteration's record gains eval_mean_reward, eval_std_reward, eval_success_rate and
        eval_ep_len_mean; with `best_model_save_path` rank 0 writes `<path>/best_model.zip` whenever the mean is strictly greater than
        every earlier one (`self.best_mean_reward`).  Evaluation does not perturb training: it consumes neither the minibatch generator
        nor the action-noise counter and updates no normaliser.  With `dist` every rank evaluates on its own eval env (its shard) and the
        record says so (eval_scope="rank"): the figures are this rank's, not agreed across ranks."""
        if eval_env is not None and eval_env is self.env:
            raise L.AmenvError("learn: eval_env must be a separate GpuWaypointEnv (evaluating on the training env would cut the rollout's episode continuity)")
        if (eval_env is None) != (not eval_freq):
            raise L.AmenvError("learn: eval_env and eval_freq go together")
        n_eval = None if eval_env is None else int(n_eval_episodes if n_eval_episodes is not None else eval_env.num_envs)
        if not hasattr(self, "best_mean_reward"):
            self.best_mean_reward = -math.inf
        next_eval = None if eval_env is None else (self.num_timesteps // int(eval_freq) + 1) * int(eval_freq)
        target = self.num_timesteps + int(total_timesteps)
        next_save = None if not save_freq else (self.num_timesteps // int(save_freq) + 1) * int(save_freq)
        while self.num_timesteps < target:
            self.env.stats(reset=True)
            self.collect_rollouts()
            ep = self.env.stats(reset=True)
            # SB3 (reset_num_timesteps=False): progress_remaining = 1 - num_timesteps / target, set after the rollout, before train()
            # (held at 0 where the last rollout overshoots the target, so that a linear schedule never turns negative)
            self._progress = max(1.0 - self.num_timesteps / float(target), 0.0)
            try:
                rec = self.train()
            finally:
                self._progress = 1.0
            n_ep = max(int(ep["episodes"]), 1)
            rec.update(timesteps=self.num_timesteps, episodes=int(ep["episodes"]), ep_rew_mean=ep["return_sum"] / n_ep,
                       ep_len_mean=ep["length_sum"] / n_ep, success_rate=ep["success"] / n_ep)
            if next_eval is not None and self.num_timesteps >= next_eval:
                mean, std, info = self._evaluate(eval_env, n_eval, eval_deterministic)
                rec.update(eval_mean_reward=mean, eval_std_reward=std, eval_success_rate=info["success_rate"], eval_ep_len_mean=info["ep_len_mean"])
                if self.world > 1:
                    rec.update(eval_scope="rank")
                if mean > self.best_mean_reward:   # SB3's EvalCallback: strictly better
                    self.best_mean_reward = mean
                    if best_model_save_path is not None and (self.dist is None or self.dist.get_rank() == 0):
                        os.makedirs(best_model_save_path, exist_ok=True)
                        self.save(os.path.join(best_model_save_path, "best_model"))
                next_eval = (self.num_timesteps // int(eval_freq) + 1) * int(eval_freq)
            self.log.append(rec)
            if log_fn is not None:
                log_fn(rec)
            if next_save is not None and self.num_timesteps >= next_save:
                if self.dist is None or self.dist.get_rank() == 0:
                    os.makedirs(save_path or ".", exist_ok=True)
                    self.save(os.path.join(save_path or ".", f"{name_prefix}_{self.num_timesteps}_steps"))
                next_save = (self.num_timesteps // int(save_freq) + 1) * int(save_freq)
        return self

    def predict(self, obs, deterministic=True):
        if self.obs_normalizer is not None:
            obs = self.obs_normalizer.normalize(obs)
        return self.policy.predict(obs, deterministic, self._gen)

    # ---- checkpoints ----------------------------------------------------------------------------
    def save(self, path):
        """A zip with SB3's member names: `policy.pth` (SB3 keys: loadable into an SB3 `ActorCriticPolicy`),
        `policy.optimizer.pth` (this class's Adam state) and `data` (hyper-parameters as plain JSON: under a schedule the CURRENT numeric
        learning_rate / clip_range / clip_range_vf -- schedules are not serialised, whoever resumes passes them again -- plus target_kl, n_updates and, with
        `adaptive_lr`, the rule's five numbers; the learning rate is the one the rule arrived at, as a float that holds its float32 exactly); with a reward normaliser one more
        member, `reward_normalizer.npz` (its `state_dict`), which `load` restores into this model's normaliser.  It is NOT a complete
        SB3 archive (SB3's `data` holds cloudpickled objects); use `policy.pth` to move weights either way."""
        path = path if str(path).endswith(".zip") else str(path) + ".zip"
        data = {k: getattr(self, k) for k in ("n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "ent_coef",
                                              "vf_coef", "max_grad_norm", "normalize_advantage", "num_timesteps", "seed", "target_kl", "n_updates", "clip_range_vf")}
        data.update(adaptive_lr=None if self.adaptive_lr is None else self.adaptive_lr.state_dict())
        data.update(format="amenv-ppo", draw=int(self._draw), learning_rate=self.optimizer.param_groups[0]["lr"], net_arch=list(self.policy.net_arch),
                    obs_dim=self.policy.obs_dim, act_dim=self.policy.act_dim)
        with zipfile.ZipFile(path, "w") as z:
            for name, obj in (("policy.pth", {k: v.detach().cpu().clone() for k, v in self.policy.state_dict().items()}),
                              ("policy.optimizer.pth", self.optimizer.state_dict())):
                buf = io.BytesIO()
                torch.save(obj, buf)
                z.writestr(name, buf.getvalue())
            z.writestr("data", json.dumps(data))
            if self.reward_normalizer is not None:   # return statistics + carried returns, plain numpy arrays (no pickle)
                buf = io.BytesIO()
                np.savez(buf, **self.reward_normalizer.state_dict())
                z.writestr("reward_normalizer.npz", buf.getvalue())
        return path

    def load_policy(self, path_or_state_dict):
        """Resume from a checkpoint's weights (`PPO.load(CHECKPOINT_PATH, ...)`, v2/rl_train.py:33-35): SB3 zip, this class's
        zip or a bare `policy.pth`.  Copies into the flat buffer in place."""
        sd = path_or_state_dict if isinstance(path_or_state_dict, dict) else ActorCritic.read_sb3_state_dict(path_or_state_dict)
        own = self.policy.state_dict()
        if set(sd) != set(own):
            raise L.AmenvError(f"checkpoint keys differ: {sorted(set(sd) ^ set(own))}")
        with torch.no_grad():
            for k, v in own.items():
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise L.AmenvError(f"{k}: checkpoint shape {tuple(sd[k].shape)} != policy {tuple(v.shape)}")
                v.copy_(torch.as_tensor(sd[k]).to(v.device))
        return self

    def load(self, path):
        """Full resume from a zip written by `save()`: weights, Adam moments / step count, learning rate (bit for bit; under `adaptive_lr` the
        rule's numbers too, into a model that was built with a rule) and the timestep counter
        (`PPO.load(CHECKPOINT_PATH, env=...)` followed by `learn`, v2/rl_train.py:33-35,56).  An SB3 archive has no optimiser state
        this class can read without unpickling: for those use `load_policy` (weights only)."""
        with zipfile.ZipFile(path if str(path).endswith(".zip") else str(path) + ".zip") as z:
            self.load_policy(torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True))
            names = z.namelist()
            data = json.loads(z.read("data")) if "data" in names else {}
            if "policy.optimizer.pth" in names and data.get("format") == "amenv-ppo":
                osd = torch.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
                cur = self.optimizer.state_dict()
                if len(osd["param_groups"]) != len(cur["param_groups"]):
                    raise L.AmenvError("optimizer state of the checkpoint does not match this optimizer")
                # copy into the live tensors: a captured update graph keeps pointing at them
                st = self.optimizer.state[self._leaf]
                src = osd["state"].get(0, {})
                if src:
                    if not st:   # Adam creates its moments lazily
                        st["step"] = torch.zeros((), dtype=torch.float32, device=self.device)
                        st["exp_avg"] = torch.zeros_like(self._leaf); st["exp_avg_sq"] = torch.zeros_like(self._leaf)
                    for k in ("step", "exp_avg", "exp_avg_sq"):
                        st[k].copy_(torch.as_tensor(src[k]).to(st[k].device))
                for g, gs in zip(self.optimizer.param_groups, osd["param_groups"]):
                    g["lr"] = gs["lr"]
            self.num_timesteps = int(data.get("num_timesteps", self.num_timesteps))
            self.n_updates = int(data.get("n_updates", self.n_updates))
            self._draw = int(data.get("draw", self._draw))   # action-noise counter: resumed rollouts draw fresh noise
            if data.get("adaptive_lr") is not None and self.adaptive_lr is not None:   # the rule's numbers, into a model built with one
                self.adaptive_lr = self._step.adaptive_lr = KlAdaptiveLr(**data["adaptive_lr"])
            if "reward_normalizer.npz" in names and self.reward_normalizer is not None:
                with np.load(io.BytesIO(z.read("reward_normalizer.npz")), allow_pickle=False) as sd:
                    self.reward_normalizer.load_state_dict({k: sd[k] for k in sd.files})
        return self


@torch.no_grad()
def clone_pid_policy(env, policy, steps=600, epochs=400, dagger_rounds=0, noise=0.15, initial_log_std=-1.0, seed=1):
    """Warm start for `PPO`: fit the actor's mean to `PidWaypointPolicy` (the reference's PID + minimum-snap baseline, HIP kernels) by behaviour
    cloning on states the PID visits (exploration noise on the executed actions, so that the data covers recoveries); with `dagger_rounds` > 0
    the STUDENT then flies while the PID labels the states it reaches, and the actor is refitted on everything collected (DAgger).  Sets
    log_std to `initial_log_std`.  Returns the final MSE.

    Why: with SB3's default initialisation PPO (the reference's hyper-parameters, v2/rl_train.py:38-53) leaves the free-fall plateau on the
    reference's quadrotor after ~35 M steps but not on the hexacopter within 150 M -- whatever its moment scaling, rotor limits, inertia,
    exploration noise or thrust bias (profiles/r03/ppo_hexa_sweep_*.json); from a cloned actor -- even one that does not yet reach a single
    waypoint itself -- it reaches > 90 % success on the hexacopter in ~55 M steps and on the hexacopter + arm (tool-point task) in 35-77 M."""
    from .baselines import PidWaypointPolicy
    pid = PidWaypointPolicy.for_env(env)
    g = torch.Generator(device=env.device).manual_seed(seed)
    X, Y = [], []

    def collect(student):
        obs = env.reset()
        done = None
        if pid.pstate is not None:
            pid.pstate[:, 13] = 1.0          # every env starts a fresh episode (new minimum-snap segment)
        for _ in range(steps):
            a = pid.predict(obs, done)
            X.append(obs.clone()); Y.append(a.clone())
            fly = policy.actor(obs) if student else a
            noisy = fly + noise * torch.randn(a.shape, device=a.device, generator=g)
            obs, _, done, _ = env.step(torch.max(torch.min(noisy, policy.action_high), policy.action_low))

    def fit():
        Xc, Yc = torch.cat(X), torch.cat(Y)
        opt = torch.optim.Adam(list(policy.mlp_extractor.policy_net.parameters()) + list(policy.action_net.parameters()), lr=1e-3)
        loss = None
        for _ in range(epochs):
            idx = torch.randint(0, Xc.shape[0], (min(16384, Xc.shape[0]),), device=Xc.device)
            with torch.enable_grad():
                loss = ((policy.actor(Xc[idx]) - Yc[idx]) ** 2).mean()
                opt.zero_grad(); loss.backward(); opt.step()
        return float(loss.detach())

    with torch.no_grad():
        collect(False)
    mse = fit()
    for _ in range(int(dagger_rounds)):
        with torch.no_grad():
            collect(True)
        mse = fit()
    with torch.no_grad():
        policy.log_std.data.fill_(float(initial_log_std))
    return mse


def reduce_evaluation(returns, counts, steps_run=None):
    """The numbers of an evaluation from `GpuWaypointEnv.evaluate_policy`'s two arrays (host arrays or tensors): returns [N, 2] (per env: sum
    and sum of squares of the counted episodes' returns), counts [N, 6] (episodes, length_sum, success, crashed, out_of_bounds, truncated).
    Returns (mean, std, info) over ALL counted episodes -- std is the population value, as `evaluate_policy` reports it -- with info =
    {episodes, ep_len_mean, success_rate, crash_rate, oob_rate, truncated_rate, steps_run}.  Raises when no episode was counted."""
    r = np.asarray(returns.cpu() if torch.is_tensor(returns) else returns, dtype=np.float64).reshape(-1, 2)
    c = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts).astype(np.int64).reshape(-1, L.EVAL_COUNT_COLS)
    tot = c.sum(0)
    k = int(tot[0])
    if k == 0:
        raise L.AmenvError("evaluate_policy: no episode finished within the step limit")
    mean = float(r[:, 0].sum()) / k
    var = max(float(r[:, 1].sum()) / k - mean * mean, 0.0)
    info = dict(episodes=k, ep_len_mean=float(tot[1]) / k, success_rate=float(tot[2]) / k, crash_rate=float(tot[3]) / k, oob_rate=float(tot[4]) / k,
                truncated_rate=float(tot[5]) / k, steps_run=None if steps_run is None else int(steps_run))
    return mean, math.sqrt(var), info


def _evaluate_fused(model, env, n_eval_episodes, deterministic, max_steps, seed=0, draw0=0):
    """evaluate_policy(fused=True): one launch, one device-to-host transfer -> (mean, std, info)."""
    policy = getattr(model, "policy", model)
    if not hasattr(policy, "flat_param"):
        raise L.AmenvError("evaluate_policy(fused=True) needs a PPO or an ActorCritic (something with flat_param); other models: fused=False")
    if policy.flat_param is None or policy.flat_param.data_ptr() != policy.log_std.data_ptr():   # (not, or no longer, the parameters' home)
        policy.flatten_()
    per_env = -(-int(n_eval_episodes) // env.num_envs)
    out = env.evaluate_policy(policy.flat_param, per_env, max_steps=max_steps, deterministic=deterministic, seed=seed, draw0=draw0,
                              obs_normalizer=getattr(model, "obs_normalizer", None), reset=True)
    # one transfer: the three arrays as raw bytes
    host = torch.cat([out["returns"].reshape(-1).view(torch.uint8), out["counts"].reshape(-1).view(torch.uint8),
                      out["steps_run"].reshape(1).view(torch.uint8)]).cpu().numpy()
    n, nb = env.num_envs, env.num_envs * 16
    returns = host[:nb].view(np.float64).reshape(n, 2)
    counts = host[nb:nb + n * 4 * L.EVAL_COUNT_COLS].view(np.int32).reshape(n, L.EVAL_COUNT_COLS)
    steps_run = int(host[nb + n * 4 * L.EVAL_COUNT_COLS:].view(np.int32)[0])
    return reduce_evaluation(returns, counts, steps_run)


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, check_every=64, max_steps=None, fused=False, return_info=False):
    """SB3 `evaluate_policy(model, env, n_eval_episodes)` (v2/rl_train.py:60) on the batched env: every env contributes the
    same number of episodes (ceil(n / num_envs), SB3's rule for vectorised envs), returns (mean, std) of the episode returns.
    `model`: a `PPO`, an `ActorCritic` or anything with `.predict(obs, deterministic)`.  The loop stays on the device; the host
    looks at the completion counters once every `check_every` steps.

    fused=True (a `PPO` or an `ActorCritic`): the whole evaluation is ONE launch (`GpuWaypointEnv.evaluate_policy`) and one device-to-host
    transfer; a `PPO`'s `obs_normalizer` is used frozen.  Same (mean, std) definition over all counted episodes, same error when none
    finished.  It evaluates the bf16 BEHAVIOUR policy of the fused rollout (the MLPs on the matrix cores), not the fp32
    modules that `predict` runs: the means differ by ~1e-2 of their scale.  return_info=True (fused only): a third value, the dict of
    `reduce_evaluation` (episodes, ep_len_mean, success_rate, crash_rate, oob_rate, truncated_rate, steps_run)."""
    if fused:
        mean, std, info = _evaluate_fused(model, env, n_eval_episodes, deterministic, max_steps)
        return (mean, std, info) if return_info else (mean, std)
    if return_info:
        raise L.AmenvError("evaluate_policy: return_info needs fused=True (the step-by-step loop keeps no end flags)")
    n = env.num_envs
    per_env = -(-int(n_eval_episodes) // n)
    obs = env.reset()
    counts = torch.zeros(n, dtype=torch.int64, device=obs.device)
    total = torch.zeros(n, dtype=torch.float64, device=obs.device)
    total_sq = torch.zeros_like(total)
    lengths = torch.zeros(n, dtype=torch.int64, device=obs.device)
    limit = max_steps if max_steps is not None else per_env * (int(env.cfg.task.max_episode_steps) + 2)
    for t in range(limit):
        obs, _, done, _ = env.step(model.predict(obs, deterministic))
        take = (done != 0) & (counts < per_env)
        r = env.ep_return.to(torch.float64)
        total += torch.where(take, r, torch.zeros_like(r))
        total_sq += torch.where(take, r * r, torch.zeros_like(r))
        lengths += torch.where(take, env.ep_len.to(torch.int64), torch.zeros_like(lengths))
        counts += take.to(torch.int64)
        if (t + 1) % check_every == 0 and bool((counts >= per_env).all()):
            break
    k = int(counts.sum())
    if k == 0:
        raise L.AmenvError("evaluate_policy: no episode finished within the step limit")
    mean = float(total.sum()) / k
    var = max(float(total_sq.sum()) / k - mean * mean, 0.0)
    return mean, math.sqrt(var)
