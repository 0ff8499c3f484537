#!/usr/bin/env python3
"""Outputs of the one-launch closed loops (amenv_rollout_policy[_norm], amenv_evaluate_policy) on the smallest shapes that reach every class of
their kernels, for tools/compare_outputs.py: run it with two builds of the library (AMENV_LIB) and the same seed, then compare the two
directories byte for byte.

    python tools/policy_outputs.py DIR [--seed 11]

Per case: the full rollout-buffer rows of an 8-step launch (obs, actions, logp, values, rewards, dones, info_bits, terminal_obs) and get_state()
behind it; max_episode_steps = 5, so every env resets inside the launch.  The cases:
  * rigid quad and hexa, v2 with 3 waypoints and v1_raw, without and with the observation normaliser, at 300 (ragged, 16 envs per workgroup),
    6200 (64) and 24700 (128) envs; all five opt-in switches on at 300 envs (the action history without the normaliser, the rest with both);
  * the arm with 3 and 2 joints at 300 (one env wavefront) and 16500 (two) envs, with 1 and 4 waypoints, on the one-lane-per-env form;
  * the lane-team and lane-quad forms (the defaults of hexa_arm and quad at 300 envs);
  * evaluate_policy, deterministic and sampled, two episodes per env, at 300 envs: rigid quad (plain, normaliser, switches) and the arm.
One .npy per array."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T = 8

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    import numpy as np
    import torch
    import rl_aerial_manipulator_amd as amd
    from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
    from rl_aerial_manipulator_amd.ppo import ActorCritic
    os.makedirs(a.dir, exist_ok=True)
    dev = torch.device("cuda", 0)

    def switches(hist):
        kw = dict(randomization=amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1)), rotor_lag=amd.RotorLag(0.015, 0.04),
                  sensor_noise=amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01), action_delay=amd.ActionDelay(0, 8))
        if hist:
            kw["action_history"] = amd.ActionHistory(2)
        return kw

    # name -> (env keywords, with the normaliser too)
    cases = {}
    for veh in ("quad", "hexa"):
        for n in (300, 6200, 24700):
            cases[f"{veh}_v2k3_{n}"] = (dict(num_envs=n, vehicle=veh, num_waypoints=3), True)
            cases[f"{veh}_v1raw_{n}"] = (dict(num_envs=n, vehicle=veh, task="v1_raw"), True)
    cases["quad_v2k3_300_switches"] = (dict(num_envs=300, vehicle="quad", num_waypoints=3, **switches(False)), True)
    cases["quad_v2k3_300_switches_hist"] = (dict(num_envs=300, vehicle="quad", num_waypoints=3, **switches(True)), False)
    for nj in (3, 2):
        for n in (300, 16500):
            for k in (1, 4):
                cases[f"arm{nj}_k{k}_{n}"] = (dict(num_envs=n, vehicle="hexa_arm", n_joints=nj, num_waypoints=k, kernel="lane"), False)
    cases["arm3_team_300"] = (dict(num_envs=300, vehicle="hexa_arm"), False)
    cases["quad_quadform_300"] = (dict(num_envs=300, vehicle="quad"), False)
    evals = {"quad_v2k3_300": True, "quad_v2k3_300_switches": True, "quad_v2k3_300_switches_hist": False, "hexa_v1raw_300": True, "arm3_k1_300": False,
             "arm2_k4_300": False}

    def policy(env):
        torch.manual_seed(7)
        pol = ActorCritic(env.obs_dim, env.act_dim).cuda().flatten_()
        with torch.no_grad():
            pol.log_std.data.fill_(-1.2)
            pol.action_net.weight.mul_(30.0)
        return pol

    def normalizer(env):   # statistics formed on the host: update() adds its fp64 partial sums with atomics, in an order that differs from run to run
        nrm = ObsNormalizer(env.obs_dim)
        x = env.observe().double().cpu().numpy()
        nrm.set(x.mean(0), x.var(0) + 0.01, env.num_envs)
        return nrm

    for name, (kw, with_norm) in cases.items():
        for tag in ("policy", "policy_norm") if with_norm else ("policy",):
            env = amd.GpuWaypointEnv(seed=a.seed, env_id_offset=1000, max_episode_steps=5, **kw)
            env.reset()
            n, od, ad = env.num_envs, env.obs_dim, env.act_dim
            pol = policy(env)
            b = dict(obs=torch.zeros(T + 1, n, od, device=dev), actions=torch.zeros(T, n, ad, device=dev), logp=torch.zeros(T, n, device=dev),
                     values=torch.zeros(T, n, device=dev), rewards=torch.zeros(T, n, device=dev), dones=torch.zeros(T, n, dtype=torch.uint8, device=dev),
                     info_bits=torch.zeros(T, n, dtype=torch.int32, device=dev), terminal_obs=torch.zeros(T, n, od, device=dev))
            nrm = normalizer(env) if tag == "policy_norm" else None
            env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, obs_normalizer=nrm, update_normalizer=False, **b)
            torch.cuda.synchronize()
            out = {f"{tag}_{k}": v for k, v in b.items()}
            out[f"{tag}_final_fstate"], out[f"{tag}_final_istate"] = env.get_state()
            if name in evals and (tag == "policy" or evals[name]):
                for det in (True, False):
                    r = env.evaluate_policy(pol.flat_param, 2, deterministic=det, seed=78, draw0=9, obs_normalizer=nrm)
                    torch.cuda.synchronize()
                    for k, v in r.items():
                        out[f"{tag}_eval_{'det' if det else 'sampled'}_{k}"] = v
                    f, i = env.get_state()
                    out[f"{tag}_eval_{'det' if det else 'sampled'}_fstate"], out[f"{tag}_eval_{'det' if det else 'sampled'}_istate"] = f, i
            if nrm is not None:
                nrm.close()
            for k, v in out.items():
                np.save(os.path.join(a.dir, f"{name}.{k}.npy"), np.atleast_1d(v.cpu().numpy()))   # (steps_run is 0-dim: compare_outputs.py views bytes)
            env.close()
    print(f"wrote {len(os.listdir(a.dir))} arrays to {a.dir}")
