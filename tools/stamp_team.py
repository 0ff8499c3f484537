#!/usr/bin/env python3
"""Lane-team step kernel (diagnostic -DAMENV_STAMPS build): phases of BOTH roles' wavefronts, with and without an episode end in the
launch, and which role a launch waits for.
  AMENV_LIB=tools/micro/libamenv_stamps.so python tools/stamp_team.py

A stamped wave fills two rows of the stamp area (16 words):
  0 start | 1 loads issued | 2 loads landed | 3 (flag) an episode ended: in this wave (integrating) / in this workgroup (helper)
  4 advance done | 5 barrier passed (integrating: and reset values taken) | 6 stores issued (helper: service done) | 7 stores acknowledged
  8 (flag) role: 0 integrating, 1 helper | 9 / 10 constant-frequency counter (100 MHz) at the first / last stamp
  11 last pre-barrier store issued (integrating; 0 in a build that stores behind the barrier) | 12 (flag, helper) an end was predicted
Words 0..7 and 11 are s_memtime clocks: comparable inside a workgroup.  Workgroups are compared on the constant-frequency counter, whose
tick is ~24 clocks; the clocks per tick are taken from the waves' own (last - first) pairs.  The stamped workgroups are spread evenly over
the grid, every wave of each."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--launches", type=int, default=1500)
a = ap.parse_args()
import torch

import rl_aerial_manipulator_amd as amd

env = amd.GpuWaypointEnv(a.envs, vehicle="hexa_arm", seed=0, kernel="team")
env.reset()
lib = C.CDLL(amd._lib.LIB_PATH)
lib.amenv_debug_stamps.argtypes = [C.c_void_p, C.c_void_p]
g = torch.Generator(device="cuda").manual_seed(1)
ring = torch.randn(16, a.envs, env.act_dim, device="cuda", generator=g) * 0.1
ring[..., 0] += 1.0
ring[..., 4:] *= 3.0
ring = ring.clamp(min=-1, max=2).contiguous()
for t in range(2000):
    env.step(ring[t % 16])
recs = []
for t in range(a.launches):
    env.step(ring[t % 16])
    buf = np.zeros((64, 8), np.uint64)
    lib.amenv_debug_stamps(env._h, buf.ctypes.data_as(C.c_void_p))
    recs.append(buf.astype(np.int64))
R = np.stack(recs, 0).reshape(len(recs), 32, 16)        # [launch, stamped wave, word]
R = R[:, R[0, :, 0] != 0, :]                            # rows no wave wrote stay zero
mw = 4 if "helper wave per 4" in env.kernel_name else 1
W = mw + 1                                              # waves of a workgroup: mw integrating, then the helper
G = R.shape[1] // W
R = R[:, :G * W].reshape(R.shape[0], G, W, 16)          # [launch, workgroup, wave, word]
assert (R[:, :, :mw, 8] == 0).all() and (R[:, :, mw, 8] == 1).all(), "role words"
I, H = R[:, :, :mw, :], R[:, :, mw, :]                  # integrating waves, helper
print(f"{env.kernel_name}\n{a.envs} envs, {a.launches} launches, {G} stamped workgroups of {mw} + 1 waves")

# ---- the integrating waves, as before (clocks from the wave's first instruction)
ended = I[..., 3] != 0
t = I - I[..., 0:1]
print(f"integrating waves: {int(ended.sum())} wave-launches with an episode end, {int((~ended).sum())} without; median clocks, none ended / ended")
for k, n_ in ((1, "loads issued, store offsets formed"), (2, "loads landed"), (4, "advance done (RK4, task, episode end)"), (11, "last pre-barrier store issued"),
              (5, "barrier passed, reset values taken"), (6, "stores issued"), (7, "drained")):
    if k == 11 and not (I[..., 11] != 0).any():
        continue
    col = t[..., k]
    print(f"   {n_:40s} {np.median(col[~ended]):8.0f} {np.median(col[ended]) if ended.any() else float('nan'):8.0f}")
span = t[..., 4] - t[..., 2]
print("compute span (loads landed -> advance done) by wave position in its workgroup: median / 99th percentile / max")
for w in range(mw):
    s = span[:, :, w]
    print(f"   wave {w}: {np.median(s):8.0f} {np.percentile(s, 99):8.0f} {s.max():8.0f}")

# ---- the helper (clocks from ITS first instruction), by whether a row of its workgroup ended
hend, hpred = H[..., 3] != 0, H[..., 12] != 0
th = H - H[..., 0:1]
print(f"helper waves: a row ended in {int(hend.sum())} workgroup-launches, none in {int((~hend).sum())}; an end was predicted in {int(hpred.sum())}; median clocks, none ended / a row ended")
for k, n_ in ((2, "loads landed"), (5, "barrier passed"), (6, "service done"), (7, "stores acknowledged")):
    col = th[..., k]
    print(f"   {n_:40s} {np.median(col[~hend]):8.0f} {np.median(col[hend]) if hend.any() else float('nan'):8.0f}")
post = H[..., 7] - H[..., 5]
for name, m in (("none ended", ~hend), ("a row ended", hend)):
    if m.any():
        print(f"   post-barrier span, {name:12s}: median {np.median(post[m]):6.0f}  90th {np.percentile(post[m], 90):6.0f}  max {post[m].max():6.0f}")

# ---- inside a workgroup (one s_memtime clock): who ends last
last_int = I[..., 7].max(axis=2)
d = H[..., 7] - last_int                                 # > 0: the helper is this workgroup's last wave
print("helper's last stamp minus the last integrating wave's, same workgroup (clocks; > 0 = the helper ends last): median / 10th / 90th percentile")
for name, m in (("none ended", ~hend), ("a row ended", hend)):
    if m.any():
        print(f"   {name:12s}: {np.median(d[m]):7.0f} {np.percentile(d[m], 10):7.0f} {np.percentile(d[m], 90):7.0f}   helper last in {100.0 * (d[m] > 0).mean():.1f} % of {int(m.sum())}")
starts = I[..., 0] - I[..., 0].min(axis=2, keepdims=True)
print("start of integrating wave w after the first of its workgroup (clocks, median):", " ".join(f"{np.median(starts[:, :, w]):.0f}" for w in range(mw)),
      "| helper:", f"{np.median(H[..., 0] - I[..., 0].min(axis=2)):.0f}")

# ---- across workgroups (the constant-frequency counter): per launch, the last wave of each role and the spread of starts
life_c, life_rt = (R[..., 7] - R[..., 0]).astype(np.float64), (R[..., 10] - R[..., 9]).astype(np.float64)
cpt = float(np.median(life_c.sum(axis=(1, 2)) / life_rt.sum(axis=(1, 2))))      # clocks per tick: whole launches' sums, so the ticks' rounding averages out
print(f"constant-frequency counter: {cpt:.1f} clocks per tick (rounding: +-1 tick per stamp)")
e_int = I[..., 10].max(axis=(1, 2)).astype(np.float64)                           # per launch: last integrating wave of the stamped workgroups
e_hlp = H[..., 10].max(axis=1).astype(np.float64)
s_all = R[..., 9].astype(np.float64)
launch_end = np.maximum(e_int, e_hlp)
any_end = hend.any(axis=1)
print("per launch, over the stamped workgroups (clocks = ticks x clocks per tick):")
print(f"   spread of wave starts (last - first): median {np.median(s_all.max(axis=(1, 2)) - s_all.min(axis=(1, 2))) * cpt:7.0f}  90th {np.percentile(s_all.max(axis=(1, 2)) - s_all.min(axis=(1, 2)), 90) * cpt:7.0f}")
wg_start = R[..., 9].min(axis=2).astype(np.float64)
print(f"   spread of workgroup starts:           median {np.median(wg_start.max(axis=1) - wg_start.min(axis=1)) * cpt:7.0f}  90th {np.percentile(wg_start.max(axis=1) - wg_start.min(axis=1), 90) * cpt:7.0f}")
print(f"   first start -> last end:              median {np.median(launch_end - s_all.min(axis=(1, 2))) * cpt:7.0f}")
for name, m in (("no stamped row ended", ~any_end), ("a stamped row ended", any_end)):
    if not m.any():
        continue
    dd = (e_hlp - e_int)[m] * cpt
    print(f"   {name:22s} ({int(m.sum()):5d} launches): helper last in {100.0 * (dd > 0).mean():5.1f} %, integrating last in {100.0 * (dd < 0).mean():5.1f} %, same tick {100.0 * (dd == 0).mean():5.1f} %;"
          f" last helper minus last integrating wave: median {np.median(dd):7.0f}  10th {np.percentile(dd, 10):7.0f}  90th {np.percentile(dd, 90):7.0f}")
