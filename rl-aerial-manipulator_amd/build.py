"""Build libamenv.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box
with the repo snapshot.  Usage: python -m build  (from the package dir) or build.build().

The library is seven sources, each compiled to an object under build/ with a depfile (hipcc -MD), in parallel, then one
link.  A source is recompiled when its object is older than a file its depfile names or than this file, where the flags live.
"""
import concurrent.futures
import os
import shutil
import subprocess
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libamenv.so")
OBJDIR = os.path.join(HERE, "build")
SOURCES = ["amenv_capi.hip", "amenv_capi_step.hip", "amenv_capi_rollout.hip", "amenv_capi_policy.hip", "amenv_capi_policy_norm.hip", "amenv_capi_eval.hip",
           "amenv_capi_train.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-ffp-contract=off", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function",
         # episode-end code adds its own lane's numbers with plain no-return atomics (usually ONE lane is active): the wave-reduction
         # the compiler would wrap around same-address atomics is a hundred instructions on a path whose cost is its instruction count
         "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]
LINK_FLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc"]
TIMES = {}   # source -> seconds of its last compile in this process (build_time records)


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm to build libamenv.so)")


def workers():
    """Compiles at a time: MAX_JOBS where it is set, else 8 -- never the machine's CPU count, which a shared box overstates."""
    return max(1, min(len(SOURCES), int(os.environ["MAX_JOBS"]) if os.environ.get("MAX_JOBS") else 8))


def _dep_files(depfile):
    """The prerequisites a make-format depfile names (relative ones are relative to csrc/, where the compiler ran)."""
    text = open(depfile).read().replace("\\\n", " ")
    return [os.path.join(CSRC, p) for rule in text.split("\n") if ":" in rule for p in rule.split(":", 1)[1].split()]


def _stale(obj):
    dep = obj[:-2] + ".d"
    if not (os.path.exists(obj) and os.path.exists(dep)):
        return True
    t = os.path.getmtime(obj)
    if os.path.getmtime(os.path.abspath(__file__)) > t:
        return True
    return any(not os.path.exists(p) or os.path.getmtime(p) > t for p in _dep_files(dep))


def _run_all(cmds, verbose):
    """cmds: {source: command}; runs them workers() at a time from csrc/, fills TIMES, raises on the first failure."""
    def one(item):
        src, cmd = item
        if verbose:
            print(" ".join(cmd), flush=True)
        t0 = time.time()
        subprocess.check_call(cmd, cwd=CSRC)
        TIMES[src] = time.time() - t0
        if verbose:
            print(f"  {src}: {TIMES[src]:.0f} s", flush=True)
    with concurrent.futures.ThreadPoolExecutor(workers()) as pool:
        list(pool.map(one, cmds.items()))


def build(force=False, verbose=False, extra_flags=(), drop_flags=(), objdir=OBJDIR, lib=LIB):
    """Compile what is stale (force: everything), link when anything was compiled or the library is missing.  extra_flags / drop_flags /
    objdir / lib: a variant of the library with other flags keeps its objects and its .so apart (tools/build_variant.py)."""
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in FLAGS if f not in drop_flags] + list(extra_flags)
    objs = {s: os.path.join(objdir, s[:-4] + ".o") for s in SOURCES}
    todo = {s: [hipcc()] + flags + ["-c", "-MD", "-MF", o[:-2] + ".d", s, "-o", o] for s, o in objs.items() if force or _stale(o)}
    _run_all(todo, verbose)
    if todo or not os.path.exists(lib) or any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs.values()):
        cmd = [hipcc()] + LINK_FLAGS + list(objs.values()) + ["-o", lib]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
    return lib


def dump_asm(outdir, extra_flags=(), verbose=False, sources=None):
    """The device assembly of every source (or of `sources`) with the build's flags: outdir/<source>.s, one per source
    (tools/asm_stats.py, tools/team_step_isa.py, the parent-vs-new comparison with tools/asm_kernel_diff.py).  Returns the paths."""
    os.makedirs(outdir, exist_ok=True)
    flags = [f for f in FLAGS if f not in ("-fPIC", "-Wall")] + list(extra_flags)
    outs = {s: os.path.join(outdir, s[:-4] + ".s") for s in (SOURCES if sources is None else sources)}
    _run_all({s: [hipcc()] + flags + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", "-o", o, s] for s, o in outs.items()}, verbose)
    return list(outs.values())


if __name__ == "__main__":
    print(build(force=True, verbose=True))
