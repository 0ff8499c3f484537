"""Step-kernel time with per-episode dynamics randomisation off and on, in the same process, hover-ish actions, two timings:
  isolated  median device time of one amenv_step launch (amenv_step_timed: HIP events around the kernel alone, host sync after each);
  graph     back-to-back launches as bench.py runs them: 64 steps captured in one graph, replayed --replays times between two events.

    python tools/dr_step_rate.py [--vehicle hexa] [--envs 4096 32768 1048576] [--kernel auto] [--steps 400]
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
    a = ap.parse_args()
    import numpy as np
    import torch
    import rl_aerial_manipulator_amd as amd
    dr = amd.DynamicsRandomization.around_one(mass=0.2, inertia=0.2, thrust=0.05)
    out = {}
    for n in a.envs:
        g = torch.Generator(device="cpu").manual_seed(0)
        acts = (torch.rand(8, n, 4, generator=g) * torch.tensor([0.4, 0.2, 0.2, 0.2]) + torch.tensor([0.8, -0.1, -0.1, -0.1])).cuda()
        for on in (False, True, False, True):   # interleaved: off, on, off, on
            env = amd.GpuWaypointEnv(n, vehicle=a.vehicle, task=a.task, seed=0, kernel=a.kernel, randomization=dr if on else None)
            env.reset()
            for t in range(a.warmup):
                env.step(acts[t % 8])
            us = [env.step_timed(acts[t % 8]) for t in range(a.steps)]
            key = f"{n}_{'dr_on' if on else 'dr_off'}"
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
        off, on = min(out[f"{n}_dr_off"]), min(out[f"{n}_dr_on"])
        goff, gon = min(out[f"{n}_dr_off_graph"]), min(out[f"{n}_dr_on_graph"])
        res[str(n)] = {"isolated_dr_off_us": off, "isolated_dr_on_us": on, "isolated_overhead_pct": 100.0 * (on - off) / off,
                       "graph_dr_off_us": goff, "graph_dr_on_us": gon, "graph_overhead_pct": 100.0 * (gon - goff) / goff,
                       "runs_off_us": out[f"{n}_dr_off"], "runs_on_us": out[f"{n}_dr_on"], "graph_runs_off_us": out[f"{n}_dr_off_graph"],
                       "graph_runs_on_us": out[f"{n}_dr_on_graph"], "kernel_off": out[f"{n}_dr_off_kernel"], "kernel_on": out[f"{n}_dr_on_kernel"]}
    print(json.dumps({"vehicle": a.vehicle, "task": a.task, "kernel": a.kernel, "steps": a.steps,
                      "timing": "isolated: median amenv_step_timed; graph: 64-step graph replays between two events; min over two interleaved runs each", "results": res}))
