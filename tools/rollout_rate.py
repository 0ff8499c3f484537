"""Closed-loop rollout rate: policy inference + Gaussian sampling + env step, everything on the GPU (what `PPO.collect_rollouts`
and `evaluate_policy` do per step).  Compares the one-launch policy forward (`amenv_policy_forward`) with the torch modules.
--one-launch: PPO's rollout collection instead -- the whole T-step closed loop as ONE launch (amenv_rollout_policy, and with
--normalize-obs amenv_rollout_policy_norm) next to the step-by-step path (one launch per operation per step), HIP-event time per step.

    python tools/rollout_rate.py [--envs 4096] [--steps 2000] [--vehicle quad] [--task v2|v1_scaled|v1_raw]
    python tools/rollout_rate.py --one-launch --task v1_raw [--normalize-obs] [--envs 4096 32768] [--rollout-steps 64]
    python tools/rollout_rate.py --one-launch --vehicle hexa_arm --n-joints 2 [--waypoints 4]
    --randomize: per-episode dynamics randomisation on (rigid vehicles; the quadrotor's one-launch rollout then runs the lane form)
    --rotor-lag TAU: first-order rotor lag on (rigid vehicles; the same rule for the quadrotor's one-launch rollout)
    --sensor-noise P V W A: sensor noise on the observations (fp32 rigid vehicles; the same rule)
    --action-delay MIN MAX: per-episode actuation latency of MIN..MAX control steps (fp32 rigid vehicles; the same rule)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--vehicle", default="quad")
    ap.add_argument("--task", default="v2", choices=["v2", "v1_scaled", "v1_raw"])
    ap.add_argument("--n-joints", type=int, default=None, help="hexa_arm: the default arm cut to its first 1..3 links")
    ap.add_argument("--waypoints", type=int, default=1, help="v2 task: waypoints per episode (1..4)")
    ap.add_argument("--one-launch", action="store_true", help="time PPO.collect_rollouts: one launch per rollout vs the step-by-step path")
    ap.add_argument("--normalize-obs", action="store_true", help="with --one-launch: an ObsNormalizer in both paths (inside the launch / per step)")
    ap.add_argument("--rollout-steps", type=int, default=64, help="with --one-launch: T steps per rollout")
    ap.add_argument("--reps", type=int, default=10, help="with --one-launch: timed rollouts per path")
    ap.add_argument("--block-size", type=int, default=0, help="amenv_config.block_size (64: the quadrotor's one-launch rollout runs the lane form, not the lane-quad one)")
    ap.add_argument("--randomize", action="store_true", help="per-episode dynamics randomisation on (mass and inertia +-20 %%, thrust +-5 %%; DESIGN 4i)")
    ap.add_argument("--rotor-lag", type=float, default=None, metavar="TAU", help="first-order rotor lag with time constant TAU seconds (DESIGN 4j)")
    ap.add_argument("--sensor-noise", type=float, nargs=4, default=None, metavar=("P", "V", "W", "A"),
                    help="sensor noise on the observations: standard deviations of position, velocity, body rate, attitude (DESIGN 4l)")
    ap.add_argument("--action-delay", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="per-episode actuation latency: each env applies the action given MIN..MAX control steps ago (DESIGN 4m)")
    ap.add_argument("--action-history", type=int, default=None, metavar="H",
                    help="append the last H (1 or 2) given action rows to every observation row (DESIGN 4n; not with --normalize-obs --one-launch)")
    a = ap.parse_args()
    import torch
    import rl_aerial_manipulator_amd as amd
    noise = None if a.sensor_noise is None else amd.SensorNoise(*a.sensor_noise)
    lag = None if a.rotor_lag is None else amd.RotorLag(a.rotor_lag)
    delay = None if a.action_delay is None else amd.ActionDelay(*a.action_delay)
    dr = amd.DynamicsRandomization.around_one(mass=0.2, inertia=0.2, thrust=0.05) if a.randomize else None
    hist = None if a.action_history is None else amd.ActionHistory(a.action_history)
    out = {}
    if a.one_launch:
        from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
        from rl_aerial_manipulator_amd.ppo import PPO
        for n in a.envs:
            for fused in (True, False):
                env = amd.GpuWaypointEnv(n, vehicle=a.vehicle, task=a.task, seed=0, n_joints=a.n_joints, num_waypoints=a.waypoints, block_size=a.block_size,
                                         randomization=dr, rotor_lag=lag, sensor_noise=noise, action_delay=delay, action_history=hist)
                norm = ObsNormalizer(env.obs_dim) if a.normalize_obs else None
                algo = PPO(env, obs_normalizer=norm, fused_rollout=fused, n_steps=a.rollout_steps, seed=0)
                algo.fused_rollout_fp32_stats = False        # time the rollout itself: no fp32 re-evaluation of the buffer behind it
                algo.bootstrap_truncated = False             # (both paths: no critic call over the terminal rows)
                for _ in range(3):
                    algo.collect_rollouts()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                ev[0].record()
                for _ in range(a.reps):
                    algo.collect_rollouts()
                ev[1].record()
                torch.cuda.synchronize()
                us = ev[0].elapsed_time(ev[1]) * 1e3 / (a.reps * a.rollout_steps)
                out[f"{n}_{'one_launch' if fused else 'step_by_step'}"] = {"us_per_step": us, "env_steps_per_s": n / us * 1e6}
                env.close()
                if norm is not None:
                    norm.close()
        print(json.dumps({"vehicle": a.vehicle, "randomize": a.randomize, "rotor_lag": a.rotor_lag, "sensor_noise": a.sensor_noise, "action_delay": a.action_delay, "action_history": a.action_history, "block_size": a.block_size, "n_joints": a.n_joints, "waypoints": a.waypoints, "task": a.task, "normalize_obs": a.normalize_obs, "rollout_steps": a.rollout_steps,
                          "loop": "PPO.collect_rollouts (policy + sample + clip + step [+ normaliser] x T, GAE)", "results": out}))
        sys.exit(0)
    for n in a.envs:
        env = amd.GpuWaypointEnv(n, vehicle=a.vehicle, task=a.task, seed=0, n_joints=a.n_joints, num_waypoints=a.waypoints, block_size=a.block_size,
                                         randomization=dr, rotor_lag=lag, sensor_noise=noise, action_delay=delay, action_history=hist)
        pol = amd.ActorCritic(env.obs_dim, env.act_dim).to(env.device).flatten_()
        for mode in ("fused", "torch"):
            obs = env.reset()
            if mode == "torch":
                pol.fused_ok = lambda o: False                        # instance override -> the torch modules
            with torch.no_grad():
                for _ in range(50):
                    obs, _, _, _ = env.step(pol.predict(obs))
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    obs, _, _, _ = env.step(torch.minimum(torch.maximum(pol.actor(obs), pol.action_low), pol.action_high))
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(16):
                        obs, _, _, _ = env.step(torch.minimum(torch.maximum(pol.actor(obs), pol.action_low), pol.action_high))
                torch.cuda.synchronize(); t1 = time.perf_counter()
                for _ in range(a.steps // 16):
                    graph.replay()
                torch.cuda.synchronize(); dg = time.perf_counter() - t1
            if mode == "torch":
                del pol.fused_ok
            out[f"{n}_{mode}"] = {"eager_us_per_step": dt / a.steps * 1e6, "graph_us_per_step": dg / (a.steps // 16 * 16) * 1e6,
                                  "graph_env_steps_per_s": n * (a.steps // 16 * 16) / dg}
        env.close()
    print(json.dumps({"vehicle": a.vehicle, "task": a.task, "randomize": a.randomize, "rotor_lag": a.rotor_lag, "sensor_noise": a.sensor_noise, "action_delay": a.action_delay, "action_history": a.action_history, "loop": "obs -> policy mean -> clip -> env.step", "results": out}))
