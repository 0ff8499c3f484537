"""The library's list of policy shapes and ActorCritic._FUSED_DIMS are one list: amenv_policy_forward,
amenv_policy_forward_mfma and amenv_ppo_mlp_step are walked over every (obs_dim, act_dim) in 1..32 x 1..8, amenv_gaussian_act and
amenv_ppo_loss_grad over act_dim 1..8, at n = 33 rows (one full 32-row tile and a ragged one).  A call returns 0 exactly for a listed shape
(act_dim 4..7) and AMENV_ERR_INVALID otherwise; an admitted call leaves its NaN-filled outputs entirely finite.

Every buffer is allocated once at the largest size of the grid (33,873 parameters = the count for 32 / 8, obs 33 x 32, actions 33 x 8, the
full workspaces), so no call of the grid, admitted or refused, can reach outside its buffers.  An admitted call gets a real packed policy of
its shape in front of the parameter buffer, and actions / old log-probabilities drawn from that policy (ratios near 1).

Last, the kernel's name is formed when it is asked for: after every setter, on and off again, amenv_kernel_name read through ctypes is
the env's kernel_name and carries exactly the suffixes of the switches that are on."""
import ctypes as C

import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.ppo import ActorCritic
from tests.policy_ref import forward_fp64, nondegenerate_policy

pytestmark = pytest.mark.gpu

N, DMAX, AMAX = 33, 32, 8
INVALID = -1   # AMENV_ERR_INVALID


def _n_params(D, A):
    trunk = 128 * D + 128 + 64 * 128 + 64 + 64 * 64 + 64
    return A + 2 * trunk + A * 64 + A + 64 + 1


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def bufs():
    dev, f32 = torch.device("cuda", 0), torch.float32
    lib = L.load()
    assert _n_params(DMAX, AMAX) == 33873
    g = torch.Generator().manual_seed(11)
    b = dict(lib=lib, stream=C.c_void_p(torch.cuda.current_stream(dev).cuda_stream),
             params=torch.zeros(_n_params(DMAX, AMAX), dtype=f32, device=dev), grad=torch.empty(_n_params(DMAX, AMAX), dtype=f32, device=dev),
             obs=torch.randn(N, DMAX, generator=g).to(dev), actions=torch.randn(N, AMAX, generator=g).to(dev),
             old_logp=torch.full((N,), -3.0, device=dev), adv=torch.randn(N, generator=g).to(dev), ret=torch.randn(N, generator=g).to(dev),
             mean=torch.empty(N, AMAX, dtype=f32, device=dev), value=torch.empty(N, dtype=f32, device=dev), stats4=torch.empty(4, dtype=f32, device=dev),
             log_std=torch.full((AMAX,), -1.0, device=dev), low=torch.full((AMAX,), -1.0, device=dev), high=torch.full((AMAX,), 1.0, device=dev),
             raw=torch.empty(N, AMAX, dtype=f32, device=dev), clipped=torch.empty(N, AMAX, dtype=f32, device=dev), logp=torch.empty(N, dtype=f32, device=dev),
             d_mean=torch.empty(N, AMAX, dtype=f32, device=dev), d_value=torch.empty(N, dtype=f32, device=dev), d_log_std=torch.empty(AMAX, dtype=f32, device=dev),
             mlp_ws=torch.empty(lib.amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device=dev),
             loss_ws=torch.empty(lib.amenv_ppo_workspace_bytes() // 8 + 1, dtype=torch.float64, device=dev))
    assert b["mlp_ws"].data_ptr() % 16 == 0 and b["loss_ws"].data_ptr() % 8 == 0
    yield b


def _stage_policy(b, D, A):
    """A real policy of shape (D, A) in front of the big buffers: its parameters, [N, D] rows, and actions / log-probabilities drawn from it."""
    pol = nondegenerate_policy(D, A, seed=100 * D + A)
    g = torch.Generator().manual_seed(D + A)
    obs = torch.randn(N, D, generator=g)
    z = torch.randn(N, A, generator=g, dtype=torch.float64)
    mean, _ = forward_fp64(pol, obs)
    ls = pol.log_std.detach().double()
    logp = (-0.5 * z * z - ls - 0.9189385332046727).sum(dim=1)
    b["params"].zero_()
    b["params"][:_n_params(D, A)] = pol.flat_param.detach().cuda()
    assert pol.flat_param.numel() == _n_params(D, A)
    b["obs"].view(-1)[:N * D] = obs.reshape(-1).cuda()
    b["actions"].view(-1)[:N * A] = (mean + ls.exp() * z).float().reshape(-1).cuda()
    b["old_logp"].copy_(logp.float())


def test_policy_entry_points_admit_exactly_the_fused_dims(bufs):
    b, lib, s = bufs, bufs["lib"], bufs["stream"]
    fused = ActorCritic._FUSED_DIMS
    assert len(fused) == 9 and all(1 <= D <= DMAX and 1 <= A <= AMAX for D, A in fused)
    for D in range(1, DMAX + 1):
        for A in range(1, AMAX + 1):
            want = 0 if (D, A) in fused else INVALID
            if want == 0:
                _stage_policy(b, D, A)
            for k in ("mean", "value", "grad", "stats4"):
                b[k].fill_(float("nan"))
            rc = lib.amenv_policy_forward(_p(b["params"]), D, A, _p(b["obs"]), N, _p(b["mean"]), _p(b["value"]), s)
            assert rc == want, ("amenv_policy_forward", D, A, rc)
            if want == 0:
                torch.cuda.synchronize()
                assert bool(torch.isfinite(b["mean"].view(-1)[:N * A]).all()) and bool(torch.isfinite(b["value"]).all()), ("amenv_policy_forward", D, A)
                b["mean"].fill_(float("nan")); b["value"].fill_(float("nan"))
            rc = lib.amenv_policy_forward_mfma(_p(b["params"]), D, A, _p(b["obs"]), N, _p(b["mean"]), _p(b["value"]), _p(b["mlp_ws"]), s)
            assert rc == want, ("amenv_policy_forward_mfma", D, A, rc)
            if want == 0:
                torch.cuda.synchronize()
                assert bool(torch.isfinite(b["mean"].view(-1)[:N * A]).all()) and bool(torch.isfinite(b["value"]).all()), ("amenv_policy_forward_mfma", D, A)
            rc = lib.amenv_ppo_mlp_step(_p(b["params"]), D, A, _p(b["obs"]), _p(b["actions"]), _p(b["old_logp"]), _p(b["adv"]), _p(b["ret"]), None, N, 0.2, 0.01, 0.5, 1,
                                        _p(b["grad"]), _p(b["stats4"]), _p(b["mlp_ws"]), s)
            assert rc == want, ("amenv_ppo_mlp_step", D, A, rc)
            if want == 0:
                torch.cuda.synchronize()
                assert bool(torch.isfinite(b["grad"][:_n_params(D, A)]).all()) and bool(torch.isfinite(b["stats4"]).all()), ("amenv_ppo_mlp_step", D, A)
    torch.cuda.synchronize()


def test_action_entry_points_admit_exactly_widths_4_to_7(bufs):
    b, lib, s = bufs, bufs["lib"], bufs["stream"]
    b["mean"].copy_(torch.linspace(-0.5, 0.5, N * AMAX).reshape(N, AMAX)); b["value"].copy_(torch.linspace(-1.0, 1.0, N))
    b["actions"].copy_(torch.linspace(0.5, -0.5, N * AMAX).reshape(N, AMAX)); b["old_logp"].fill_(-3.0)
    for A in range(1, AMAX + 1):
        want = 0 if 4 <= A <= 7 else INVALID
        for k in ("raw", "clipped", "logp", "d_mean", "d_value", "d_log_std", "stats4"):
            b[k].fill_(float("nan"))
        rc = lib.amenv_gaussian_act(_p(b["mean"]), _p(b["log_std"]), _p(b["low"]), _p(b["high"]), _p(b["raw"]), _p(b["clipped"]), _p(b["logp"]), N, A, 7, 3, 0, s)
        assert rc == want, ("amenv_gaussian_act", A, rc)
        rc = lib.amenv_ppo_loss_grad(_p(b["mean"]), _p(b["value"]), _p(b["log_std"]), _p(b["actions"]), _p(b["old_logp"]), _p(b["adv"]), _p(b["ret"]), N, A, 0.2, 0.01, 0.5, 1,
                                     _p(b["d_mean"]), _p(b["d_value"]), _p(b["d_log_std"]), _p(b["stats4"]), _p(b["loss_ws"]), s)
        assert rc == want, ("amenv_ppo_loss_grad", A, rc)
        torch.cuda.synchronize()
        if want == 0:
            assert all(bool(torch.isfinite(b[k].view(-1)[:N * A]).all()) for k in ("raw", "clipped", "d_mean")), A
            assert all(bool(torch.isfinite(b[k]).all()) for k in ("logp", "d_value", "stats4")) and bool(torch.isfinite(b["d_log_std"][:A]).all()), A


def test_kernel_name_follows_every_setter():
    env = amd.GpuWaypointEnv(130, seed=3, kernel="lane")
    switches = [("randomization", amd.DynamicsRandomization(mass=(1.5, 1.5)), " +dr"), ("rotor_lag", amd.RotorLag(0.03, 0.05), " +lag"),
                ("sensor_noise", amd.SensorNoise(position=0.02), " +noise"), ("action_delay", amd.ActionDelay(2, 2), " +delay"),
                ("action_history", amd.ActionHistory(2), " +history 2")]
    suffixes = [s for _, _, s in switches]

    def name():
        n = env.lib.amenv_kernel_name(env._h).decode()
        assert n == env.kernel_name
        return n

    base = name()
    assert not any(s.strip() in base for s in suffixes), base
    for attr, value, suffix in switches:
        getattr(env, "set_" + attr)(value)
        assert name() == base + suffix, (attr, name())
        getattr(env, "set_" + attr)(None)
        assert name() == base, (attr, name())
    for attr, value, _ in switches:       # all five on: the suffixes in the library's order
        getattr(env, "set_" + attr)(value)
    assert name() == base + "".join(suffixes)
    env.close()
