#!/usr/bin/env python3
"""Static counts of the lane-team step kernel's front, from the gfx950 assembly (needs no GPU): per instantiation of step_kernel_team the
vector loads of the integrating path and of the helper path, the scalar-load batches an integrating wave waits for in front of its first
vector load, the VALU instructions between its last load and the first wait for loaded data (the derivation of the lane constants and
the store plumbing), registers and scratch.
  python tools/team_step_isa.py [extra hipcc flags]  > profiles/<dir>/team_step_isa.txt
  python tools/team_step_isa.py --asm FILE           (an assembly file made before)

How the paths are told apart: the integrating path is the fall-through of the role branch, so the first vector load in file order is
its first; the last conditional scalar branch in front of that load is the role branch and its target starts the helper path, which
runs to the end of the kernel.  Checked here: s_setprio (integrating waves only) lies on the integrating side, and nowhere else."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rl_aerial_manipulator_amd.build as B

args = sys.argv[1:]
if args[:1] == ["--asm"]:
    asm = args[1]
else:
    (asm,) = B.dump_asm(os.path.join(tempfile.gettempdir(), "amenv_team_step"), extra_flags=args, sources=["amenv_capi_step.hip"])   # the source of the step kernels
lines = open(asm).read().split("\n")
VLOAD = re.compile(r"^\s+(global_load|buffer_load|flat_load|scratch_load)_\w+")
VSTORE = re.compile(r"^\s+(global_store|buffer_store|flat_store)_\w+")
starts = [i for i, l in enumerate(lines) if l.startswith("_ZN9amenv_dev16step_kernel_team") and l.split(":")[0].endswith("E") and ":" in l]
for i in starts:
    name = lines[i].split(":")[0]
    end = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
    code_end = next(k for k in range(i, end) if lines[k].strip().startswith(".section") or lines[k].strip().startswith(".p2align 6"))
    body = lines[i:code_end]
    meta = "\n".join(lines[code_end:end])
    m = re.search(r"step_kernel_teamI(\w)Li6ELi(\d)E", name)
    first_v = next(k for k, l in enumerate(body) if VLOAD.match(l))
    role = max(k for k in range(first_v) if re.match(r"^\s+s_cbranch_scc[01]\s", body[k]))
    label = body[role].split()[1]
    helper_at = next(k for k, l in enumerate(body) if l.startswith(label + ":"))
    assert helper_at > first_v, "the helper path is expected behind the integrating path"
    main, helper = body[:helper_at], body[helper_at:]
    assert any("s_setprio" in l for l in main) and not any("s_setprio" in l for l in helper), "role branch not identified"
    mloads = [l.split()[0] for l in main if VLOAD.match(l)]
    hloads = [l.split()[0] for l in helper if VLOAD.match(l)]
    # scalar-load batches in front of the first vector load: waits on lgkmcnt that follow at least one s_load
    batches, pending = 0, False
    for l in body[:first_v]:
        if re.match(r"^\s+s_load_", l):
            pending = True
        elif "s_waitcnt" in l and "lgkmcnt" in l and pending:
            batches, pending = batches + 1, False
    unwaited = pending
    last_v = max(k for k, l in enumerate(main) if VLOAD.match(l) and k < first_v + 64)
    wait_v = next(k for k in range(last_v, len(main)) if "s_waitcnt" in main[k] and "vmcnt" in main[k])
    valu_between = sum(1 for l in main[last_v:wait_v] if re.match(r"^\s+v_", l))
    valu_front = sum(1 for l in body[:first_v] if re.match(r"^\s+v_", l))
    g = lambda key: re.search(key + r" (\d+)", meta).group(1)
    n_scratch = sum(1 for l in body if re.match(r"^\s+scratch_", l))
    print(f"step_kernel_team<{'float' if m.group(1) == 'f' else 'double'}, 6, MW={m.group(2)}>")
    print(f"  integrating path: {len(mloads)} vector loads ({', '.join(f'{n} x {k}' for k, n in sorted({k: mloads.count(k) for k in set(mloads)}.items()))}), "
          f"{sum(1 for l in main if VSTORE.match(l))} vector stores")
    print(f"  helper path:      {len(hloads)} vector loads ({', '.join(f'{n} x {k}' for k, n in sorted({k: hloads.count(k) for k in set(hloads)}.items()))}); "
          f"the first {min(3, len(hloads))} unconditional (P, V, int plane), the rest on the episode-end / totals branches")
    print(f"  in front of the integrating wave's first vector load: {batches} scalar-load batch(es) waited for"
          f"{' (+ scalar loads issued, not waited for)' if unwaited else ''}, {valu_front} VALU instructions")
    print(f"  between its last front load and the first wait for loaded data: {valu_between} VALU instructions")
    print(f"  vgpr {g('.amdhsa_next_free_vgpr')}  sgpr {g('.amdhsa_next_free_sgpr')}  private segment {g('.amdhsa_private_segment_fixed_size')} B  scratch instructions {n_scratch}")
