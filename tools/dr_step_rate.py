"""Step-kernel time with per-episode dynamics randomisation or, with --rotor-lag TAU, the first-order rotor lag or,
with --sensor-noise P V W A, the sensor noise on the observations or, with --action-delay MIN MAX, the per-episode actuation latency
 and / or, with --action-history H, the action history in the observation rows or, with --rotor-failure P, the per-episode
rotor failure (both sides run with the randomisation, so "off" is the +dr kernel with the failure's branch not taken) off and on, in the same process, alternating, hover-ish actions, two timings:
  isolated  median device time of one amenv_step launch (amenv_step_timed: HIP events around the kernel alone, host sync after each);
  graph     back-to-back launches as bench.py runs them: 64 steps captured in one graph, replayed --replays times between two events.

    python tools/dr_step_rate.py [--vehicle hexa] [--envs 4096 32768 1048576] [--kernel auto] [--steps 400] [--rotor-lag 0.015 | --sensor-noise 0.02 0.05 0.02 0.01 | --action-delay 0 8] [--action-history 2] [--rotor-failure 0.5] [--repeats 2]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicle", default="hexa")
    ap.add_argument("--task", default="v2", choices=["v2", "v1_scaled", "v1_raw"])
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768, 1048576])
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rotor-lag", type=float, default=None, metavar="TAU", help="compare the rotor lag (time constant TAU seconds) off / on instead of the randomisation")
    ap.add_argument("--sensor-noise", type=float, nargs=4, default=None, metavar=("P", "V", "W", "A"),
                    help="compare the sensor noise (standard deviations of position, velocity, body rate, attitude) off / on instead of the randomisation")
    ap.add_argument("--action-delay", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="compare the per-episode actuation latency (MIN..MAX control steps) off / on instead of the randomisation")
    ap.add_argument("--action-history", type=int, default=None, metavar="H",
                    help="the on side also appends the last H (1 or 2) given action rows to every observation row (DESIGN 4n); alone, or on top of --action-delay")
    ap.add_argument("--rotor-failure", type=float, default=None, metavar="P",
                    help="compare the per-episode rotor failure (probability P, onset 50..400, remaining 0..0.5) off / on, both sides with the randomisation")
    ap.add_argument("--repeats", type=int, default=2, help="off / on pairs per env count (the minimum of each side is compared, every run is listed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rl_aerial_manipulator_amd as amd
    if sum(x is not None for x in (a.rotor_lag, a.sensor_noise, a.action_delay, a.rotor_failure)) > 1:
        ap.error("--rotor-lag, --sensor-noise, --action-delay and --rotor-failure are compared one at a time")
    noise = None if a.sensor_noise is None else amd.SensorNoise(*a.sensor_noise)
    delay = None if a.action_delay is None else amd.ActionDelay(*a.action_delay)
    hist = None if a.action_history is None else amd.ActionHistory(a.action_history)
    fail = None if a.rotor_failure is None else amd.RotorFailure(probability=a.rotor_failure, onset=(50, 400), remaining=(0.0, 0.5))
    if hist is not None and (a.rotor_lag is not None or noise is not None or fail is not None):
        ap.error("--action-history goes alone or with --action-delay")
    dr = amd.DynamicsRandomization.around_one(mass=0.2, inertia=0.2, thrust=0.05) if a.rotor_lag is None and noise is None and delay is None and hist is None else None
    lag = None if a.rotor_lag is None else amd.RotorLag(a.rotor_lag)
    what = "fail" if fail is not None else "delay_history" if delay is not None and hist is not None else "history" if hist is not None else "delay" if delay is not None else ("noise" if noise is not None else ("dr" if lag is None else "lag"))
    out = {}
    for n in a.envs:
        g = torch.Generator(device="cpu").manual_seed(0)
        acts = (torch.rand(8, n, 4, generator=g) * torch.tensor([0.4, 0.2, 0.2, 0.2]) + torch.tensor([0.8, -0.1, -0.1, -0.1])).cuda()
        for on in (False, True) * a.repeats:   # interleaved: off, on, off, on
            env = amd.GpuWaypointEnv(n, vehicle=a.vehicle, task=a.task, seed=0, kernel=a.kernel, randomization=dr if on or fail is not None else None, rotor_failure=fail if on else None, rotor_lag=lag if on else None,
                                     sensor_noise=noise if on else None, action_delay=delay if on else None, action_history=hist if on else None)
            env.reset()
            for t in range(a.warmup):
                env.step(acts[t % 8])
            us = [env.step_timed(acts[t % 8]) for t in range(a.steps)]
            key = f"{n}_{what}_{'on' if on else 'off'}"
            out.setdefault(key, []).append(float(np.median(us)))
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for t in range(3):
                    env.step(acts[t % 8])
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for t in range(64):
                    env.step(acts[t % 8])
            g.replay()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.replays):
                g.replay()
            ev[1].record()
            torch.cuda.synchronize()
            out.setdefault(key + "_graph", []).append(ev[0].elapsed_time(ev[1]) * 1e3 / (64 * a.replays))
            del g
            out[key + "_kernel"] = env.kernel_name
            env.close()
    res = {}
    for n in a.envs:
        k = f"{n}_{what}"
        off, on = min(out[k + "_off"]), min(out[k + "_on"])
        goff, gon = min(out[k + "_off_graph"]), min(out[k + "_on_graph"])
        res[str(n)] = {f"isolated_{what}_off_us": off, f"isolated_{what}_on_us": on, "isolated_overhead_pct": 100.0 * (on - off) / off,
                       f"graph_{what}_off_us": goff, f"graph_{what}_on_us": gon, "graph_overhead_pct": 100.0 * (gon - goff) / goff,
                       "runs_off_us": out[k + "_off"], "runs_on_us": out[k + "_on"], "graph_runs_off_us": out[k + "_off_graph"],
                       "graph_runs_on_us": out[k + "_on_graph"], "kernel_off": out[k + "_off_kernel"], "kernel_on": out[k + "_on_kernel"]}
    print(json.dumps({"vehicle": a.vehicle, "task": a.task, "kernel": a.kernel, "steps": a.steps, "compared": what, "rotor_lag": a.rotor_lag, "sensor_noise": a.sensor_noise, "action_delay": a.action_delay, "action_history": a.action_history, "rotor_failure": a.rotor_failure,
                      "timing": "isolated: median amenv_step_timed; graph: 64-step graph replays between two events; min over the interleaved runs of each side", "results": res}))
