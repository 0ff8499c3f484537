#!/usr/bin/env python3
"""Outputs of every admitted switch set of the rigid kernels, for tools/compare_outputs.py: run it with two builds of the
library and the same seed, then compare the two directories byte for byte.

    python tools/switch_outputs.py DIR [--seed 11] [--envs 130]

For each of the nine sets (none; randomisation; randomisation with every combination of rotor lag, sensor noise and actuation latency) and
the four with the action history (one and two rows, each without and with the latency, all other switches on) on quad v2 K=1 with kernel
auto / lane / helper, hexa v2 K=3 on lane and quad v1_raw on helper, and for the three sets that are built in fp64 on quad v2 K=1 lane: 8 steps,
an 8-step rollout, and (fp32) an 8-step closed-loop rollout without and -- where it is built: not with the history -- with the observation
normaliser, then the state and every switch's side state.  One more set, `dr_lag_noise_delay_fail`, has the rotor failure on top of
the four: a library without amenv_set_rotor_failure is compared on the others (--no-fail leaves the set out).  One .npy per array."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CONFIGS = {"quad_v2_auto": dict(vehicle="quad", kernel="auto"), "quad_v2_lane": dict(vehicle="quad", kernel="lane"),
           "quad_v2_helper": dict(vehicle="quad", kernel="helper"), "hexa_v2k3_lane": dict(vehicle="hexa", kernel="lane", num_waypoints=3),
           "quad_v1raw_helper": dict(vehicle="quad", kernel="helper", task="v1_raw")}
F64 = {"quad_v2_lane_f64": dict(vehicle="quad", kernel="lane", dtype="f64")}
SETS = [""] + ["dr" + lag + noise + delay for delay in ("", "_delay") for noise in ("", "_noise") for lag in ("", "_lag")]
SETS += [f"dr_lag_noise{delay}_hist{rows}" for rows in (1, 2) for delay in ("", "_delay")]
FAIL_SET = "dr_lag_noise_delay_fail"
SETS_F64 = ["", "dr", "dr_lag"]
T = 8

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--envs", type=int, default=130)
    ap.add_argument("--no-fail", action="store_true", help="leave the rotor-failure set out (the file list of a library from before DESIGN 4y)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rl_aerial_manipulator_amd as amd
    from rl_aerial_manipulator_amd.obs_norm import ObsNormalizer
    from rl_aerial_manipulator_amd.ppo import ActorCritic
    os.makedirs(a.dir, exist_ok=True)
    n, dev = a.envs, torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(a.seed)
    acts = (torch.rand(2 * T, n, 4, generator=g) * torch.tensor([0.6, 0.4, 0.4, 0.4]) + torch.tensor([0.7, -0.2, -0.2, -0.2])).to(dev).contiguous()
    for cname, ckw in list(CONFIGS.items()) + list(F64.items()):
        for sname in (SETS_F64 if cname in F64 else SETS + ([] if a.no_fail else [FAIL_SET])):
            more = dict(rotor_failure=amd.RotorFailure(probability=0.7, onset=(2, 9), remaining=(0.0, 0.5))) if "fail" in sname else {}
            env = amd.GpuWaypointEnv(n, seed=a.seed, env_id_offset=1000, max_episode_steps=12, **ckw,
                                     randomization=amd.DynamicsRandomization(mass=(0.8, 1.2), inertia=(0.7, 1.3), thrust=(0.9, 1.1)) if "dr" in sname else None,
                                     rotor_lag=amd.RotorLag(0.015, 0.04) if "lag" in sname else None,
                                     sensor_noise=amd.SensorNoise(position=0.02, velocity=0.05, rate=0.02, attitude=0.01) if "noise" in sname else None,
                                     action_delay=amd.ActionDelay(0, 8) if "delay" in sname else None,
                                     action_history=amd.ActionHistory(int(sname[-1])) if "hist" in sname else None, **more)
            out = {"reset_obs": env.reset().clone()}
            steps = [[x.clone() for x in env.step(acts[t])] + [env.terminal_obs.clone()] for t in range(T)]
            for k, name in enumerate(("obs", "reward", "done", "info", "terminal_obs")):
                out["step_" + name] = torch.stack([s[k] for s in steps])
            for k, v in env.rollout(acts[T:]).items():
                out["rollout_" + k] = v
            od = env.obs_dim
            torch.manual_seed(7)
            pol = ActorCritic(od, 4).cuda().flatten_()
            with torch.no_grad():
                pol.log_std.data.fill_(-1.2)
                pol.action_net.weight.mul_(30.0)
            for tag in () if cname in F64 else ("policy",) if "hist" in sname else ("policy", "policy_norm"):
                b = dict(obs=torch.zeros(T + 1, n, od, device=dev), actions=torch.zeros(T, n, 4, device=dev), logp=torch.zeros(T, n, device=dev),
                         values=torch.zeros(T, n, device=dev), rewards=torch.zeros(T, n, device=dev), dones=torch.zeros(T, n, dtype=torch.uint8, device=dev))
                nrm = None
                if tag == "policy_norm":
                    nrm = ObsNormalizer(od)
                    x = env.observe().double().cpu().numpy()      # statistics formed on the host: update() adds its fp64 partial sums with
                    nrm.set(x.mean(0), x.var(0), n)               # atomics, in an order that differs from run to run in the last bit
                env.rollout_policy(pol.flat_param, T, seed=77, draw0=5, obs_normalizer=nrm, **b)
                torch.cuda.synchronize()
                if nrm is not None:
                    nrm.close()
                for k, v in b.items():
                    out[f"{tag}_{k}"] = v
            out["final_fstate"], out["final_istate"] = env.get_state()
            if "lag" in sname:
                out["final_rotor_state"] = env.rotor_state()
            if "delay" in sname or "hist" in sname:
                out["final_delay_d"], out["final_delay_recent"] = env.action_delay_state()
            if "fail" in sname:
                out["final_fail_plan"], out["final_fail_factors"] = env.rotor_failure_state()
            out["kernel_name"] = torch.tensor(list(env.kernel_name.encode()), dtype=torch.uint8)
            for k, v in out.items():
                np.save(os.path.join(a.dir, f"{cname}.{sname or 'none'}.{k}.npy"), v.cpu().numpy())
            env.close()
    print(f"wrote {len(os.listdir(a.dir))} arrays to {a.dir}")
