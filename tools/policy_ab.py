#!/usr/bin/env python3
"""A/B timing of the one-launch closed loops between two builds of libamenv.so (tools/ab_kernel.py's scheme: every measurement is a child
process with AMENV_LIB set, rounds interleaved A / B / A / B by the parent).

    python tools/policy_ab.py --libs tools/micro/libamenv_parent.so rl-aerial-manipulator_amd/libamenv.so --rounds 5 --out profiles/r19/policy_ab.json

Cases: us per step of the one-launch rollout (tools/rollout_rate.py --one-launch) for quad v1_raw with the normaliser and hexa v2 at 4096 and
32768 envs, hexa v2 on 3 waypoints at 4096 / 16384 / 32768, the 2-joint arm with 4 waypoints at 20000 and 32768 envs; us per step of the
evaluation launch (tools/eval_rate.py) at 4096 and 256 envs.
Per case and library: the rounds, their median and spread (max - min); `within` = B's median exceeds A's by no more than A's spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROLLOUT = {"quad_v1raw_norm": ["--task", "v1_raw", "--normalize-obs", "--envs", "4096", "32768"],
           "hexa_v2": ["--vehicle", "hexa", "--envs", "4096", "32768"],                                # (one waypoint: the lane-quad form, a control)
           "hexa_v2k3": ["--vehicle", "hexa", "--waypoints", "3", "--envs", "4096", "16384", "32768"],   # the rigid form without the normaliser, NE = 16 / 64 / 128
           "arm2_k4": ["--vehicle", "hexa_arm", "--n-joints", "2", "--waypoints", "4", "--envs", "20000", "32768"]}


def child(lib, cmd, limit):
    o = subprocess.run([sys.executable] + cmd, env=dict(os.environ, AMENV_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=limit)
    line = [ln for ln in o.stdout.splitlines() if ln.startswith("{")]
    if o.returncode != 0 or not line:
        raise SystemExit(f"FAILED ({o.returncode}) {lib} {' '.join(cmd)}\n{o.stderr[-2000:]}")   # nothing more is started on the device
    return json.loads(line[-1])


def one_round(lib, limit):
    got = {}
    for name, args in ROLLOUT.items():
        r = child(lib, [os.path.join(TOOLS, "rollout_rate.py"), "--one-launch"] + args, limit)["results"]
        for k, v in r.items():
            if k.endswith("_one_launch"):
                got[f"rollout_{name}_{k.split('_')[0]}"] = v["us_per_step"]
    r = child(lib, [os.path.join(TOOLS, "eval_rate.py"), "--envs", "4096", "256"], limit)["results"]
    for n, v in r.items():
        got[f"eval_launch_{n}"] = v["eval_launch_us_per_step"]
    return got


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, required=True, metavar=("A", "B"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rounds = {lib: [] for lib in a.libs}
    for r in range(a.rounds):
        for lib in a.libs:
            rounds[lib].append(one_round(lib, a.child_timeout))
            print(f"round {r} {os.path.basename(lib)} {json.dumps(rounds[lib][-1])}", flush=True)
    A, B = a.libs
    cases = {}
    for k in rounds[A][0]:
        xa, xb = [x[k] for x in rounds[A]], [x[k] for x in rounds[B]]
        ma, mb, spread = statistics.median(xa), statistics.median(xb), max(xa) - min(xa)
        cases[k] = dict(a_rounds_us=xa, b_rounds_us=xb, a_median_us=ma, b_median_us=mb, a_spread_us=spread, within=mb - ma <= spread)
        print(f"{k:32s} A {ma:9.3f} (spread {spread:7.3f})  B {mb:9.3f}  {'within' if cases[k]['within'] else 'EXCEEDS'}")
    doc = dict(what="us per step, one-launch rollout (rollout_rate.py --one-launch) and evaluation launch (eval_rate.py); one child process per library and "
               "measurement, rounds interleaved A / B; within: median(B) - median(A) <= max(A) - min(A)", a=A, b=B, rounds=a.rounds, cases=cases)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(c["within"] for c in cases.values()) else 1)
