"""Does the action history help under latency?  (evidence, not a gate.)

The reference quadrotor trained from random weights with examples/rl_train_gpu.py's reference recipe (256 envs x 512 steps, 90 M steps,
one launch per rollout) under ActionDelay(0, 2) + RotorLag(0.015), once with ActionHistory(2) in the observation and once without, per
seed; every trained policy is then flown by evaluate_policy at the FIXED delays 0, 1 and 2 (lag on), and the success rate of the episodes
that ended is recorded.

    python tools/action_history_study.py --seeds 0 1 2 --out profiles/r12/action_history_study.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--arms", nargs="+", default=["history", "plain"], choices=["history", "plain"])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--n-steps", type=int, default=512)
    ap.add_argument("--timesteps", type=int, default=90_000_000)
    ap.add_argument("--eval-episodes", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rl_aerial_manipulator_amd as amd
    runs = []
    for seed in a.seeds:
        for arm in a.arms:
            env = amd.GpuWaypointEnv(a.envs, vehicle="quad", seed=seed, rotor_lag=amd.RotorLag(0.015), action_delay=amd.ActionDelay(0, 2),
                                     action_history=amd.ActionHistory(2) if arm == "history" else None)
            model = amd.PPO(env, learning_rate=2e-4, n_steps=a.n_steps, batch_size=a.envs * a.n_steps // 128, n_epochs=12, gamma=0.995, gae_lambda=0.9,
                            clip_range=0.2, ent_coef=5e-4, fused_rollout=True, seed=seed)
            t0 = time.time()
            model.learn(a.timesteps)
            rec = {"seed": seed, "arm": arm, "obs_dim": env.obs_dim, "learn_seconds": round(time.time() - t0, 1),
                   "train_success_rate_last_10_iterations": sum(r["success_rate"] for r in model.log[-10:]) / max(1, len(model.log[-10:]))}
            for d in (0, 1, 2):
                env.set_action_delay(amd.ActionDelay(d))
                env.reset()                       # every env starts an episode with the fixed delay
                env.stats(reset=True)
                mean_reward, _ = amd.evaluate_policy(model, env, n_eval_episodes=a.eval_episodes)
                s = env.stats()
                rec[f"eval_delay_{d}"] = {"episodes": s["episodes"], "success": s["success"], "crashed": s["crashed"],
                                          "success_rate": s["success"] / max(1, s["episodes"]), "mean_reward": float(mean_reward)}
            print(json.dumps(rec), flush=True)
            runs.append(rec)
            env.close()
    out = {"command": " ".join(sys.argv), "recipe": "quad, ActionDelay(0, 2) + RotorLag(0.015), PPO 256 envs x 512 steps, fused rollout, 12 epochs, lr 2e-4, ent 5e-4",
           "timesteps": a.timesteps, "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
