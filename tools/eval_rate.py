"""Evaluation rate: `evaluate_policy` step by step (one launch per operation per step, the host looking at the counters every
64 steps) against `evaluate_policy(fused=True)` (amenv_evaluate_policy: one launch, one transfer), alternated in ONE process on the same env
and checkpoint, one episode per env; and the evaluation launch against amenv_rollout_policy on a one-lane twin over the same number of steps.
Host clock around a device synchronise; the median of --reps runs each.

    python tools/eval_rate.py [--envs 4096 256] [--reps 5] [--out profiles/r09/eval_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import rl_aerial_manipulator_amd as amd
    from rl_aerial_manipulator_amd.ppo import ActorCritic, evaluate_policy

    def clock(f):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "policy_2300000.npz"))
    pol = ActorCritic.from_sb3({k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("_")}, device="cuda").flatten_()
    results = {}
    for n in a.envs:
        env = amd.GpuWaypointEnv(n, seed=0)
        twin = amd.GpuWaypointEnv(n, seed=0, block_size=64)          # amenv_rollout_policy in the one-lane form
        for _ in range(2):                                           # warm-up of both paths
            evaluate_policy(pol, env, n_eval_episodes=n)
            evaluate_policy(pol, env, n_eval_episodes=n, fused=True)
        step_s, fused_s, launch_s, roll_s, steps_run, figures = [], [], [], [], [], []
        for _ in range(a.reps):                                      # alternated: drift of the clocks hits both alike
            dt, (m0, s0) = clock(lambda: evaluate_policy(pol, env, n_eval_episodes=n))
            step_s.append(dt)
            dt, (m1, s1, info) = clock(lambda: evaluate_policy(pol, env, n_eval_episodes=n, fused=True, return_info=True))
            fused_s.append(dt); steps_run.append(info["steps_run"]); figures.append(dict(step_by_step_mean=m0, fused_mean=m1, fused_success_rate=info["success_rate"]))
            # the launch alone against the rollout launch over the same number of steps (both from a reset, deterministic vs the rollout's sampling)
            env.reset()
            dt, out = clock(lambda: env.evaluate_policy(pol.flat_param, 1, reset=False))
            T = int(out["steps_run"])
            launch_s.append(dt / T)
            twin.reset()
            b = dict(obs=torch.empty(T + 1, n, 20, device="cuda"), actions=torch.empty(T, n, 4, device="cuda"), logp=torch.empty(T, n, device="cuda"),
                     values=torch.empty(T, n, device="cuda"), rewards=torch.empty(T, n, device="cuda"), dones=torch.empty(T, n, dtype=torch.uint8, device="cuda"))
            dt, _ = clock(lambda: twin.rollout_policy(pol.flat_param, T, 0, 0, **b))
            roll_s.append(dt / T)
            del b
        med = statistics.median
        results[str(n)] = dict(step_by_step_s=med(step_s), fused_s=med(fused_s), speedup=med(step_s) / med(fused_s), steps_run=steps_run,
                               step_by_step_all_s=step_s, fused_all_s=fused_s,
                               eval_launch_us_per_step=med(launch_s) * 1e6, rollout_launch_us_per_step=med(roll_s) * 1e6,
                               eval_launch_all_us=[x * 1e6 for x in launch_s], rollout_launch_all_us=[x * 1e6 for x in roll_s], last=figures[-1])
        env.close(); twin.close()
    doc = dict(what="evaluate_policy, one episode per env, quadrotor v2, checkpoint tests/golden/policy_2300000.npz; host clock around a device synchronise, "
               "median of the repeats; *_launch_us_per_step: the evaluation launch vs amenv_rollout_policy (one-lane form) over the same number of steps",
               reps=a.reps, results=results)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
