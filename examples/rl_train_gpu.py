"""The reference's training entry (initial-implementation-v2/rl_train.py:22-64) on the GPU-resident stack.

    python examples/rl_train_gpu.py [--envs 4096] [--timesteps 4100000] [--resume ppo_model_2300000_steps.zip]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/rl_train_gpu.py ...
    python examples/rl_train_gpu.py --task v1_raw --normalize-obs [--fused-rollout]      # initial-implementation-v1/rl_train_vecN.py

Same hyper-parameters as the reference (lr 2e-4, 12 epochs, gamma .995, lambda .9, clip .2, ent 5e-4 -- 1e-4 when resuming,
:35 -- MLP [128,64,64] tanh); the rollout is `envs x n_steps` instead of `8 x 2048`, so n_steps / batch_size are rescaled to
keep the reference's 16,384-sample rollouts x 128-sample minibatches ratio (128 minibatches per epoch).
--task v1_scaled / v1_raw: the recipe of v1/rl_train_vecN.py instead (10 epochs, ent .01, the 17-D v1 env); --normalize-obs wraps the env
as its VecNormalize(norm_obs=True, norm_reward=False) does, and the statistics are saved next to the checkpoint (<save>_vec_normalize.npz,
GpuVecNormalize.save's format).  With --fused-rollout the normaliser runs inside the launch and its statistics are frozen for each
rollout.

Defaults = the run recorded in profiles/r01/ppo_from_scratch.json: 256 envs x 512 steps, 90 M steps, ~10 minutes on one MI355X, > 90 % of
episodes successful after 39 M steps.  Learning progress follows the number of Adam updates (1536 per iteration here), not the number of samples:
thousands of envs with proportionally larger minibatches collect samples faster but learn no sooner.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--n-steps", type=int, default=512)
    ap.add_argument("--timesteps", type=int, default=90_000_000)         # rl_train.py:56 uses 4.1 M per run, ~15 M in total
    ap.add_argument("--resume", default=None, help="SB3 zip / policy.pth to start from (rl_train.py:33-35)")
    ap.add_argument("--save", default="waypoint_controller_gpu")         # rl_train.py:57
    ap.add_argument("--vehicle", default="quad")
    ap.add_argument("--n-joints", type=int, default=None, help="hexa_arm: the default arm cut to its first 1..3 links (obs 23 + 2 n, actions 4 + n)")
    ap.add_argument("--task", default="v2", choices=["v2", "v1_scaled", "v1_raw"],
                    help="v2: rl_train.py's env; v1_scaled / v1_raw: the v1 env files (rl_train_vecN.py imports rl_env = v1_raw) with rl_train_vecN.py's recipe")
    ap.add_argument("--normalize-obs", action="store_true", help="observation normaliser (VecNormalize(norm_obs=True, norm_reward=False), rl_train_vecN.py:10-11)")
    ap.add_argument("--norm-reward", action="store_true", help="return-based reward scaling (VecNormalize(norm_reward=True), SB3's default: gamma .99, clip 10); "
                    "the statistics travel inside the saved zip; ep_rew_mean and the final evaluation stay raw")
    ap.add_argument("--seed", type=int, default=0, help="env reset stream, initial weights and action noise (one run = one seed: PPO on this task is seed-sensitive)")
    ap.add_argument("--moment-scale", type=float, default=None, help="N m per unit moment action (amenv_vehicle.moment_scale; the reference quadrotor: 0.1)")
    ap.add_argument("--fused-rollout", action="store_true", help="collect every rollout as ONE launch (amenv_rollout_policy: the policy on bf16 matrix cores inside the env loop; "
                                                                 "log-probs / values of the buffer re-evaluated in fp32); quadrotor, hexacopter, hexacopter + arm")
    for q, what in (("mass", "the body's mass (actions keep the nominal scaling)"), ("inertia", "the body's inertia"), ("thrust", "each rotor's thrust")):
        ap.add_argument(f"--randomize-{q}", type=float, default=0.0, metavar="F",
                        help=f"per-episode dynamics randomisation: scale {what} by a factor drawn from [1 - F, 1 + F] (rigid vehicles; DESIGN 4i)")
    ap.add_argument("--rotor-lag", type=float, default=None, metavar="TAU",
                    help="first-order rotor lag with time constant TAU seconds, up and down (rigid vehicles; the hexacopter model's motors: 0.015; DESIGN 4j)")
    ap.add_argument("--sensor-noise", type=float, nargs=4, default=None, metavar=("P", "V", "W", "A"),
                    help="sensor noise on the observations: standard deviations of position (m), velocity (m/s), body rate (rad/s) and attitude (rad) "
                         "(fp32 rigid vehicles; DESIGN 4l)")
    ap.add_argument("--action-delay", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="per-episode actuation latency: each env applies the action it was given MIN..MAX control steps of 5 ms ago (0..8; "
                         "fp32 rigid vehicles; DESIGN 4m)")
    ap.add_argument("--action-history", type=int, default=None, metavar="H",
                    help="append the last H (1 or 2) action rows each env was given to its observation rows: the commands still in flight under "
                         "--action-delay / --rotor-lag (fp32 rigid vehicles; not with --normalize-obs --fused-rollout; DESIGN 4n)")
    ap.add_argument("--rate-control", type=float, nargs="*", default=None, metavar="X",
                    help="body-rate actions: entries 1..3 of an action are rate commands and a rate loop inside the step forms the moments (what a PX4 "
                         "offboard controller accepts).  No values: max_rate 5 5 2.5 rad/s, gain 25 25 10 1/s; or six: RX RY RZ GX GY GZ (fp32 rigid "
                         "vehicles; not with --warm-start-pid; DESIGN 4v)")
    ap.add_argument("--rotor-failure", type=float, default=None, metavar="P",
                    help="per-episode rotor failure: with probability P an episode loses one rotor (drawn per episode) at a control step drawn from "
                         "50..400, which from then on delivers 0..50 %% of its thrust; not observed (rigid vehicles; pair it with --action-history; DESIGN 4y)")
    ap.add_argument("--target-kl", type=float, default=None, metavar="X",
                    help="SB3's target_kl: leave an update once a minibatch's approx_kl exceeds 1.5 X (decided on the GPU, no extra synchronisation; one rank only)")
    ap.add_argument("--lr-schedule", default="constant", choices=["constant", "linear", "adaptive"],
                    help="linear: learning_rate = 2e-4 * progress_remaining (SB3's linear schedule), evaluated once per iteration; adaptive: 2e-4 is the starting "
                         "value and every minibatch's approx_kl moves it (amd.KlAdaptiveLr, rsl_rl's rule, on the GPU with no extra synchronisation; one rank "
                         "only; DESIGN 4u)")
    ap.add_argument("--desired-kl", type=float, default=0.01, metavar="X", help="--lr-schedule adaptive: the approx_kl the rule steers to (the rate moves outside [X / 2, 2 X])")
    ap.add_argument("--clip-range-vf", type=float, default=None, metavar="C", help="SB3's clipped value loss: the value prediction moves at most C from the rollout's value")
    ap.add_argument("--eval-freq", type=int, default=None, metavar="STEPS",
                    help="evaluate the deterministic policy every STEPS env steps on a separate eval env, in one launch (SB3's EvalCallback; DESIGN 4s): the "
                         "learning curve gains eval_mean_reward / eval_success_rate, the best model goes to <save>_best/best_model.zip")
    ap.add_argument("--eval-envs", type=int, default=1024, help="envs of the eval env (one episode each per evaluation); also used by the final evaluation")
    ap.add_argument("--log-json", default=None, help="write the learning curve (one record per iteration) and the final evaluation to this file")
    ap.add_argument("--warm-start-pid", type=int, default=None, metavar="DAGGER_ROUNDS",
                    help="initialise the actor by behaviour cloning of the PID + minimum-snap baseline (amd.clone_pid_policy; 0 = plain cloning, k = k DAgger rounds). "
                         "Needed for the hexacopter vehicles: from SB3's default initialisation PPO does not leave the free-fall plateau there (profiles/r03/ppo_hexa_sweep_*.json)")
    a = ap.parse_args()
    if a.rate_control is not None and len(a.rate_control) not in (0, 6):
        ap.error("--rate-control takes no values or six: RX RY RZ GX GY GZ")
    import torch
    import rl_aerial_manipulator_amd as amd
    from rl_aerial_manipulator_amd import sharding
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    sh = sharding.shard_from_env(a.envs)
    dist = sharding.init_process_group("nccl", torch.device("cuda", local))
    cfg = None
    if a.moment_scale is not None:
        cfg = amd._lib.default_config(a.vehicle, a.envs, a.task, n_joints=a.n_joints)
        cfg.vehicle.moment_scale = a.moment_scale
        cfg.seed, cfg.env_id_offset = a.seed, sh.env_id_offset

    def make_env(n, seed, offset, config):   # the training env, and the eval env that mirrors its vehicle, task and switches under a seed of its own
        e = amd.GpuWaypointEnv(n, device=local, vehicle=a.vehicle, seed=seed, env_id_offset=offset, config=config, task=a.task, n_joints=a.n_joints)
        if a.randomize_mass or a.randomize_inertia or a.randomize_thrust:
            e.set_randomization(amd.DynamicsRandomization.around_one(mass=a.randomize_mass, inertia=a.randomize_inertia, thrust=a.randomize_thrust))
        if a.rotor_lag is not None:
            e.set_rotor_lag(amd.RotorLag(a.rotor_lag))
        if a.sensor_noise is not None:
            e.set_sensor_noise(amd.SensorNoise(*a.sensor_noise))
        if a.action_delay is not None:
            e.set_action_delay(amd.ActionDelay(*a.action_delay))
        if a.action_history is not None:
            e.set_action_history(amd.ActionHistory(a.action_history))
        if a.rate_control is not None:
            e.set_rate_control(amd.RateControl(a.rate_control[:3], a.rate_control[3:]) if a.rate_control else amd.RateControl())
        if a.rotor_failure is not None:
            e.set_rotor_failure(amd.RotorFailure(probability=a.rotor_failure, onset=(50, 400), remaining=(0.0, 0.5)))
        return e

    env = make_env(a.envs, a.seed, sh.env_id_offset, cfg)
    ecfg = None
    if cfg is not None:
        ecfg = amd._lib.Config.from_buffer_copy(cfg)
        ecfg.num_envs, ecfg.seed, ecfg.env_id_offset = a.eval_envs, a.seed + 1_000_003, sh.rank * a.eval_envs
    eval_env = make_env(a.eval_envs, a.seed + 1_000_003, sh.rank * a.eval_envs, ecfg)
    norm = amd.ObsNormalizer(env.obs_dim, device=local) if a.normalize_obs else None
    v1 = a.task != "v2"     # rl_train_vecN.py: 10 epochs, ent .01 (v2/rl_train.py: 12 epochs, ent 5e-4)
    lr = (lambda progress_remaining: 2e-4 * progress_remaining) if a.lr_schedule == "linear" else 2e-4
    rule = amd.KlAdaptiveLr(desired_kl=a.desired_kl) if a.lr_schedule == "adaptive" else None
    model = amd.PPO(env, learning_rate=lr, adaptive_lr=rule, clip_range_vf=a.clip_range_vf, target_kl=a.target_kl, n_steps=a.n_steps, batch_size=a.envs * a.n_steps // 128, n_epochs=10 if v1 else 12, gamma=0.995,
                    gae_lambda=0.9, clip_range=0.2, ent_coef=0.01 if v1 else (1e-4 if a.resume else 5e-4), dist=dist, fused_rollout=a.fused_rollout,
                    seed=a.seed, obs_normalizer=norm, reward_normalizer=amd.RewardNormalizer(env.num_envs, device=local) if a.norm_reward else None)
    if a.resume:
        model.load_policy(a.resume)
    elif a.warm_start_pid is not None:
        mse = amd.clone_pid_policy(env, model.policy, dagger_rounds=a.warm_start_pid)
        if dist is not None:        # every rank cloned on its own shard: continue from rank 0's actor
            for p_ in model.policy.parameters():
                dist.broadcast(p_.data, src=0)
        if sh.rank == 0:
            print(f"warm start: actor cloned from PidWaypointPolicy (mse {mse:.4f}, {a.warm_start_pid} DAgger rounds), log_std = -1", flush=True)
    curve = []

    def show(r):
        curve.append({k: (round(v, 8 if k in ("approx_kl", "learning_rate") else 4) if isinstance(v, float) else v) for k, v in r.items()})
        print(curve[-1], flush=True)

    import time
    t0 = time.time()
    model.learn(a.timesteps, log_fn=show if sh.rank == 0 else None, **(dict(eval_env=eval_env, eval_freq=a.eval_freq, best_model_save_path=a.save + "_best")
                                                                     if a.eval_freq else {}))
    seconds = time.time() - t0
    if sh.rank == 0:
        print("saved", model.save(a.save))
        if norm is not None:    # env.save("vec_normalize") of rl_train_vecN.py, in GpuVecNormalize.save's .npz format
            import numpy as np
            mean, var, count = norm.get()
            np.savez(a.save + "_vec_normalize.npz", mean=mean, var=var, count=count, clip_obs=norm.clip_obs, epsilon=norm.epsilon)
            print("saved", a.save + "_vec_normalize.npz")
        # rl_train.py:60-61, in one launch on the eval env: the deterministic bf16 behaviour policy, the normaliser frozen
        if norm is not None and a.action_history is not None:   # (the one combination the fused forms are not built for)
            (mean_reward, std_reward), eval_info = amd.evaluate_policy(model, eval_env, n_eval_episodes=max(10, a.eval_envs)), None
        else:
            mean_reward, std_reward, eval_info = amd.evaluate_policy(model, eval_env, n_eval_episodes=max(10, a.eval_envs), fused=True, return_info=True)
        print(f"Mean reward: {mean_reward} +/- {std_reward}  {eval_info}")
        if curve and curve[-1].get("success_rate", 1.0) < 0.5 and a.warm_start_pid is None and not a.resume:
            print("this run stayed on the hover plateau (about one seed in six does within 90 M steps, profiles/r03/ppo_seed_sweep_quad/): "
                  "try another --seed, or --warm-start-pid 3 (actor cloned from the PID baseline), which leaves it from the first iterations")
        if a.log_json:
            import json
            first90 = next((c["timesteps"] for c in curve if c["success_rate"] > 0.9), None)
            with open(a.log_json, "w") as f:
                json.dump({"command": " ".join(sys.argv), "learn_seconds": seconds, "timesteps": a.timesteps, "timesteps_to_90pct_success": first90,
                           "final_success_rate_mean_of_last_10_iterations": sum(c["success_rate"] for c in curve[-10:]) / max(1, len(curve[-10:])),
                           "n_updates": model.n_updates, "iterations_stopped_early_by_target_kl": sum(c["kl_early_stop"] for c in curve),
                           "evaluate_policy_mean_reward": mean_reward, "evaluate_policy_std_reward": std_reward, "evaluate_policy_info": eval_info,
                           "eval_curve": [{k: c[k] for k in ("timesteps", "eval_mean_reward", "eval_std_reward", "eval_success_rate", "eval_ep_len_mean")}
                                          for c in curve if "eval_mean_reward" in c],
                           "best_eval_mean_reward": model.best_mean_reward if a.eval_freq else None, "curve_every_20th_iteration": curve[::20]}, f, indent=1)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
