#!/usr/bin/env python3
"""Instruction mix of the gfx950 kernels: hipcc -S the library and count per kernel.
Usage: python tools/asm_stats.py [filter-substring] [--asm FILE]   (--asm: count an assembly file made before instead of compiling)"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_aerial_manipulator_amd.build as B

out = "/tmp/amenv.s"
if "--asm" in sys.argv:
    k = sys.argv.index("--asm")
    out = sys.argv[k + 1]
    del sys.argv[k:k + 2]
else:   # the library's own flags (build.FLAGS), assembly instead of a shared object
    subprocess.check_call([B.hipcc()] + [f for f in B.FLAGS if f not in ("-shared", "-fPIC", "-Wall")] +
                          ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", "-o", out, "amenv_capi.hip"], cwd=B.CSRC)
filt = sys.argv[1] if len(sys.argv) > 1 else "step_kernelIf"
lines = open(out).read().split("\n")
starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if l.startswith("_ZN9amenv_dev") and ":" in l]
for (i, name), nxt in zip(starts, starts[1:] + [(len(lines), "")]):
    if filt not in name:
        continue
    body = lines[i:nxt[0]]
    end = next((k for k, l in enumerate(body) if ".end_amdhsa_kernel" in l), len(body))
    ins = [l.strip().split()[0] for l in body[:end] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    c = collections.Counter(ins)
    grp = lambda p: sum(n for k, n in c.items() if k.startswith(p))
    meta = "\n".join(body[:end])
    vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta)
    sg = re.search(r"\.amdhsa_next_free_sgpr (\d+)", meta)
    print(f"{name[:72]}\n  total {len(ins)}  valu {grp('v_')}  (pk {grp('v_pk')}, trans {sum(c[k] for k in c if re.match(r'v_(rcp|rsq|sqrt|exp|log|sin|cos)', k))})"
          f"  salu {grp('s_')} (s_load {grp('s_load')}, waitcnt {c['s_waitcnt']})  gload {grp('global_load')}  gstore {grp('global_store')}"
          f"  ds {grp('ds_')}  scratch {grp('scratch_')}  vgpr {vg.group(1) if vg else '?'} sgpr {sg.group(1) if sg else '?'}")
