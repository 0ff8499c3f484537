"""Timing of the fused PPO training kernels.

  python tools/ppo_mlp_rate.py                      forward + backward of a minibatch, torch modules against the fused kernel; the forward alone
  python tools/ppo_mlp_rate.py --ab OTHER_LIB.so    one whole minibatch step (amenv_ppo_mlp_step + amenv_ppo_adam_step) of this tree's library against
                                                    another build of it (e.g. the parent commit's), alternating in ONE process, at 65,536 and
                                                    1,024 samples; with --json FILE the table is written there.  Both libraries are called
                                                    through the plain entry points; this tree's also through the _ctl ones, gate open and gate shut
                                                    (what a minibatch step costs after target_kl tripped: four early-exit launches), with the
                                                    KL-adaptive Adam step (amenv_ppo_adam_step_adapt) and with the clipped value loss
                                                    (amenv_ppo_mlp_step_vclip), DESIGN 4u.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd.ppo import MinibatchStep, ActorCritic


def paths():
    for (D, A) in ((29, 7), (20, 4)):
        n = 65536
        pol = ActorCritic(D, A).cuda().flatten_()
        opt = torch.optim.Adam([pol.flat_param.requires_grad_(True)], lr=1e-3)
        obs = torch.randn(n, D, device="cuda"); actions = torch.randn(n, A, device="cuda"); olp = torch.randn(n, device="cuda") * 0.1 - 5
        adv = torch.randn(n, device="cuda"); ret = torch.randn(n, device="cuda")
        for fused in (False, True):
            step = MinibatchStep(pol, opt, use_graph=False, fused_mlp=fused)
            for _ in range(3): step._forward_backward(obs, actions, olp, adv, ret)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): step._forward_backward(obs, actions, olp, adv, ret)
            e1.record(); torch.cuda.synchronize()
            print(f"D={D} A={A} n={n} fused_mlp={fused}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per forward+backward")

    # the forward passes alone (amenv_policy_forward_mfma through ActorCritic.forward_fused): the rollout buffer's re-evaluation, a 32768-env policy step
    for n in (32768, 1048576):
        pol = ActorCritic(29, 7).cuda().flatten_()
        obs = torch.randn(n, 29, device="cuda")
        with torch.no_grad():
            for _ in range(3): pol.forward_fused(obs)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): pol.forward_fused(obs)
            e1.record(); torch.cuda.synchronize()
        print(f"forward only, D=29 A=7 n={n}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per call (weight packing + mlp_forward_kernel)")


_P = C.c_void_p
_MLP = [_P, C.c_int32, C.c_int32] + [_P] * 6 + [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int32, _P, _P, _P]
_ADAM = [_P] * 5 + [C.c_int64, _P, _P, _P]


def _bind(path, new):
    lib = C.CDLL(path)
    lib.amenv_ppo_mlp_workspace_bytes.restype = C.c_size_t
    lib.amenv_ppo_mlp_step.argtypes, lib.amenv_ppo_adam_step.argtypes = _MLP + [_P], _ADAM + [_P]
    if hasattr(lib, "amenv_ppo_ctl_arm"):
        lib.amenv_ppo_mlp_step_ctl.argtypes, lib.amenv_ppo_adam_step_ctl.argtypes = _MLP + [_P, _P], _ADAM + [_P, _P]
        lib.amenv_ppo_ctl_arm.argtypes = [_P, C.c_float, _P]
    if new:
        lib.amenv_ppo_adam_step_adapt.argtypes = _ADAM + [_P, C.POINTER(amd._lib.PpoLrRule), _P]
        lib.amenv_ppo_mlp_step_vclip.argtypes = _MLP + [_P, _P, C.c_float, _P]
    return lib


def ab(other, reps, rounds, out):
    here = amd._lib.LIB_PATH
    libs = {"other": _bind(other, False), "this": _bind(here, True)}
    D, A = 29, 7
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    table = {}
    for n in (65536, 1024):
        torch.manual_seed(0)
        pol = ActorCritic(D, A).cuda().flatten_()
        P0 = pol.flat_param.detach().clone()
        obs = torch.randn(n, D, device="cuda"); actions = torch.randn(n, A, device="cuda"); olp = torch.randn(n, device="cuda") * 0.1 - 9
        adv = torch.randn(n, device="cuda"); ret = torch.randn(n, device="cuda")
        old_values = torch.randn(n, device="cuda") * 0.5
        rule = amd.KlAdaptiveLr().struct()
        k = P0.numel()
        grad, m, v = (torch.zeros(k, device="cuda") for _ in range(3))
        stp = torch.zeros((), device="cuda")
        stats = torch.zeros(6, device="cuda"); hyper = torch.tensor([2e-4, 0.9, 0.999, 1e-5, 0.5, 1.0], device="cuda")
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda"); ctl = torch.zeros(16, dtype=torch.int32, device="cuda")
        ws = torch.empty(libs["this"].amenv_ppo_mlp_workspace_bytes() // 8 + 2, dtype=torch.float64, device="cuda")
        prm = pol.flat_param.detach()

        def one(lib, use_ctl):
            a = (p(prm), D, A, p(obs), p(actions), p(olp), p(adv), p(ret), None, n, 0.2, 5e-4, 0.5, 1, p(grad), p(stats), p(ws))
            b = (p(prm), p(grad), p(m), p(v), p(stp), k, p(hyper), C.c_void_p(stats.data_ptr() + 16), p(ticket))
            if use_ctl == "adapt":
                assert lib.amenv_ppo_mlp_step_ctl(*a, p(ctl), None) == 0 and lib.amenv_ppo_adam_step_adapt(*b, p(ctl), C.byref(rule), None) == 0
            elif use_ctl == "vclip":
                assert lib.amenv_ppo_mlp_step_vclip(*a, p(ctl), p(old_values), 0.2, None) == 0 and lib.amenv_ppo_adam_step_ctl(*b, p(ctl), None) == 0
            elif use_ctl:
                assert lib.amenv_ppo_mlp_step_ctl(*a, p(ctl), None) == 0 and lib.amenv_ppo_adam_step_ctl(*b, p(ctl), None) == 0
            else:
                assert lib.amenv_ppo_mlp_step(*a, None) == 0 and lib.amenv_ppo_adam_step(*b, None) == 0

        def timed(lib, use_ctl, limit):
            prm.copy_(P0); m.zero_(); v.zero_(); stp.zero_(); hyper[0] = 2e-4
            if use_ctl:
                assert lib.amenv_ppo_ctl_arm(p(ctl), limit, None) == 0
            for _ in range(5): one(lib, use_ctl)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): one(lib, use_ctl)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3

        other_ctl = hasattr(libs["other"], "amenv_ppo_ctl_arm")      # (a parent from before the control block has no _ctl entry points)
        cases = [("other plain", "other", False, 0.0), ("this plain", "this", False, 0.0), ("other plain (again)", "other", False, 0.0)]
        if other_ctl:
            cases += [("other ctl, gate open", "other", True, 0.0)]
        cases += [
                 ("this ctl, gate open", "this", True, 0.0), ("this ctl, gate shut", "this", True, 1e-12),
                 ("this ctl + adam_step_adapt", "this", "adapt", 0.0), ("this mlp_step_vclip + ctl", "this", "vclip", 0.0)]
        if other_ctl:
            cases += [("other ctl, gate open (again)", "other", True, 0.0)]
        res = {name: [] for name, *_ in cases}
        for _ in range(rounds):                       # alternating: every round visits every case once
            for name, which, use_ctl, limit in cases:
                res[name].append(timed(libs[which], use_ctl, limit))
        table[str(n)] = {name: dict(median_us=round(statistics.median(x), 2), min_us=round(min(x), 2), max_us=round(max(x), 2)) for name, x in res.items()}
        for name, r in table[str(n)].items():
            print(f"n={n:6d} {name:28s} median {r['median_us']:8.2f} us  [{r['min_us']:.2f} .. {r['max_us']:.2f}] per minibatch step ({rounds} rounds x {reps} steps)")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(dict(shape=[D, A], reps=reps, rounds=rounds, this=os.path.basename(here), other=os.path.basename(other), us_per_minibatch_step=table), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.ab:
        ab(a.ab, a.reps, a.rounds, a.json)
    else:
        paths()
