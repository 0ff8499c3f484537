"""Plain references for the hand-written policy kernels (importable on CPU; the GPU tests run the same code on cuda tensors):

  * nondegenerate_policy: an ActorCritic whose biases and log_std are all non-zero, distinct and of both signs (SB3's orthogonal init
    zeroes every bias, which hides a dropped or permuted bias from any test that uses it);
  * forward_fp64:         mean / value of the MLPs in fp64, no rounding;
  * forward_bf16_model:   fp64 arithmetic on the operands AS THE ONE-LAUNCH ROLLOUT KERNELS ROUND THEM (amenv_*_policy.hpp): bf16 weights,
                          bf16 layer-1 inputs (two bf16 parts for the rigid vehicles), bf16 tanh outputs, fp32 biases of layers 2 / 3 and
                          of the heads, the layer-1 bias as an extra weight column against an input column of 1;
  * philox4x32 / philox_normals_fp64: Philox4x32-10 (Random123) and the samplers' Box-Muller mapping, vectorised numpy, fp64.
"""
import math

import numpy as np
import torch

from rl_aerial_manipulator_amd.ppo import ActorCritic

HEAD_BIAS = [0.9, -0.35, 0.2, -0.6, 0.45, -0.15, 0.3]
LOG_STD = [-0.4, -1.6, -0.9, -1.3, -0.6, -1.9, -1.1]
VALUE_BIAS = 2.5


def nondegenerate_policy(D, A, seed, device="cpu", w1_scale=2.0):
    """ActorCritic(D, A) (orthogonal weights from `seed`), flattened, with: every trunk bias from U(-0.4, 0.4); head biases HEAD_BIAS[:A]
    (distinct, both signs); value bias 2.5; log_std LOG_STD[:A] (distinct, non-monotone); action_net.weight x 30 (actions of order one, as
    a trained controller's); both first layers' weights x w1_scale (so the second bf16 part of the rigid forms' first layer matters)."""
    torch.manual_seed(seed)
    pol = ActorCritic(D, A).to(device)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for net in (pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net):
            for k in (0, 2, 4):
                b = net[k].bias
                b.copy_((torch.rand(b.shape, generator=g, dtype=torch.float64) * 0.8 - 0.4).to(b))
            net[0].weight.mul_(w1_scale)
        pol.action_net.weight.mul_(30.0)
        pol.action_net.bias.copy_(torch.tensor(HEAD_BIAS[:A]))
        pol.value_net.bias.fill_(VALUE_BIAS)
        pol.log_std.copy_(torch.tensor(LOG_STD[:A]))
    return pol.flatten_()


def _layers(pol, net):
    trunk = pol.mlp_extractor.policy_net if net == "pi" else pol.mlp_extractor.value_net
    head = pol.action_net if net == "pi" else pol.value_net
    return [(trunk[k].weight.detach(), trunk[k].bias.detach()) for k in (0, 2, 4)], (head.weight.detach(), head.bias.detach())


@torch.no_grad()
def forward_fp64(pol, obs):
    """(mean [n, A], value [n]) of the fp32 parameters in fp64 arithmetic, no rounding anywhere."""
    x0 = obs.detach().double()
    out = []
    for net in ("pi", "vf"):
        trunk, (Wh, bh) = _layers(pol, net)
        x = x0
        for W, b in trunk:
            x = torch.tanh(x @ W.double().T + b.double())
        out.append(x @ Wh.double().T + bh.double())
    return out[0], out[1][:, 0]


def _bf16(t, on):
    return t.bfloat16().double() if on else t.double()


def split_two_part(x):
    """x (fp32) -> (hi, lo) = (bf16(x), bf16(x - bf16(x))), as the rigid forms split the first layer's inputs and weights (the difference is
    exact in fp32); returned as fp64."""
    x = x.float()
    hi = x.bfloat16()
    return hi.double(), (x - hi.float()).bfloat16().double()


@torch.no_grad()
def forward_bf16_model(pol, obs, two_part_first_layer, rounding=True):
    """(mean [n, A], value [n]) in fp64 arithmetic on the operands as the one-launch rollout kernels round them (rounding=False: fp64 of the
    unrounded fp32 operands, i.e. forward_fp64).
      layer 1: W1 gets its bias as an extra column, x an extra column of 1.  Arm forms (team, lane): sum bf16(W) bf16(x).  Rigid forms (quad,
               rigid): bf16(W) bf16(x) + bf16(W) bf16(x - bf16(x)) + bf16(W - bf16(W)) bf16(x) (amenv_quad_policy.hpp layer 1); the bias
               column's x is 1, so its lo(x) = 0;
      every tanh output rounded to bf16 (round to nearest even, as v_cvt_pk_bf16_f32);
      layers 2 / 3 and the heads: bf16 weights, fp32 biases."""
    x = obs.detach().float()
    ones = torch.ones(x.shape[0], 1, dtype=x.dtype, device=x.device)
    xa = torch.cat([x, ones], 1)
    out = []
    for net in ("pi", "vf"):
        trunk, (Wh, bh) = _layers(pol, net)
        (W1, b1) = trunk[0]
        Wa = torch.cat([W1.float(), b1.float()[:, None]], 1)
        if not rounding:
            pre = xa.double() @ Wa.double().T
        elif two_part_first_layer:
            xh, xl = split_two_part(xa)
            wh, wl = split_two_part(Wa)
            pre = xh @ wh.T + xl @ wh.T + xh @ wl.T
        else:
            pre = _bf16(xa, True) @ _bf16(Wa, True).T
        h = _bf16(torch.tanh(pre), rounding)
        for W, b in trunk[1:]:
            h = _bf16(torch.tanh(h @ _bf16(W, rounding).T + b.double()), rounding)
        out.append(h @ _bf16(Wh, rounding).T + bh.double())
    return out[0], out[1][:, 0]


# ---- Philox4x32-10 and the samplers' normals ------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 (Random123) on broadcastable arrays of 32-bit words; returns the four output words (uint64 arrays holding uint32)."""
    k0, k1, c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _U32 for v in (k0, k1, c0, c1, c2, c3))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0 = (k0 + np.uint64(_W0)) & _U32
        k1 = (k1 + np.uint64(_W1)) & _U32
    return c0, c1, c2, c3


def philox_normals_fp64(seed, gid, draw, A):
    """The N(0, 1) draws of every sampler (amenv_gaussian_act, the one-launch rollouts) in fp64: Philox4x32-10 keyed
    (seed_lo ^ 0x5bd1e995, seed_hi ^ 0x27d4eb2f) with counter (gid_lo, gid_hi, draw mod 2^32, block); of each word pair (a, b),
    u1 = ((a >> 8) + 1) 2^-24, u2 = (b >> 8) 2^-24, rad = sqrt(-2 ln u1); entry 4 block + 2 pair = rad cos(2 pi u2), the next one
    rad sin(2 pi u2) (amenv_train.hpp gaussian_act_kernel).  gid, draw: broadcastable integer arrays; returns shape (..., A)."""
    seed = int(seed)
    gid = np.asarray(gid, dtype=np.int64).astype(np.uint64)
    draw = np.asarray(draw, dtype=np.int64).astype(np.uint64) & _U32
    gid, draw = np.broadcast_arrays(gid, draw)
    k0, k1 = (seed & 0xFFFFFFFF) ^ 0x5BD1E995, ((seed >> 32) & 0xFFFFFFFF) ^ 0x27D4EB2F
    z = np.empty(gid.shape + (4 * ((A + 3) // 4),), np.float64)
    for b in range((A + 3) // 4):
        w = philox4x32(k0, k1, gid & _U32, gid >> np.uint64(32), draw, b)
        for p in range(2):
            u1 = ((w[2 * p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
            u2 = (w[2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
            rad = np.sqrt(-2.0 * np.log(u1))
            z[..., 4 * b + 2 * p] = rad * np.cos(2.0 * math.pi * u2)
            z[..., 4 * b + 2 * p + 1] = rad * np.sin(2.0 * math.pi * u2)
    return z[..., :A]


def gaussian_logp_fp64(z, log_std):
    """sum_k (-z_k^2 / 2 - log_std_k - ln(2 pi) / 2), fp64 (DiagGaussianDistribution.log_prob at raw = mean + exp(log_std) z)."""
    z = np.asarray(z, np.float64)
    return (-0.5 * z * z - np.asarray(log_std, np.float64) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
