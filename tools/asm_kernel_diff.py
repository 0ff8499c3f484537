#!/usr/bin/env python3
"""Compare two sets of device assembly files (hipcc --cuda-device-only -S, same flags) kernel by kernel.

    python tools/asm_kernel_diff.py A B [--fold-bools N] [--list-same] > report.txt

A and B are each one .s file, several joined by commas, or a directory (every .s in it: what build.dump_asm writes, one file per source
of the library).  The kernels of a side's files are merged; a kernel name met twice on one side is an error (exit status 2): every kernel
of the library is compiled in exactly one source.

A kernel is its text from the entry label to the function's end label (instructions, local labels), its kernel descriptor, the
compiler's occupancy comment and its entry in the amdhsa.kernels metadata (.kernarg_segment_size, every argument's offset and size,
register / scratch / LDS numbers).  Kernels are matched by demangled name without the parameter list.  Only two things are normalised:
the kernel's own symbol, and the function index inside local labels (.LBB12_3, .Lfunc_end12, .Ltmp.., BB12_3 in loop comments).

--fold-bools N: a kernel of A whose template argument list ends in N bools is matched to the kernel of B that has ONE unsigned argument in
their place, the bools read as a bit mask (first bool = bit 0): `k<float, 4, true, true, false, false>` -> `k<float, 4, 3u>`.

Prints the counts, every kernel that is in one file only, and for every kernel that differs both sets of resource numbers and the first
differing line; exit status 1 unless the two files hold the same kernels with identical text and metadata.

--no-block-names: drop the IR block names the compiler prints as comments behind labels (`.LBB3_15: ; %_ZN..bodyILb0EEE...exit`, `; %bb.67: ;
%...exit1051.i`): they carry the mangled names of INLINED functions, so a new defaulted template parameter or argument of a __forceinline__
body renames them in kernels whose instructions did not move.  Everything that is not such a comment is still compared.

--brief, for a library whose kernels differ by the hundred: one line per differing kernel with the resource numbers that moved (`a>b`; every
number of RES and the occupancy that is not listed is equal), the differing kernels in which none moved counted per kernel name, and with
--list-same the identical kernels counted per kernel name."""
import argparse
import glob
import os
import re
import subprocess
import sys

RES = ("sgpr_count", "vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count",
       "kernarg_segment_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(dem):
    """`void ns::k<a, b>(params)` -> `ns::k<a, b>`"""
    s = (dem[5:] if dem.startswith("void ") else dem).replace("(anonymous namespace)", "{anonymous}")
    depth = 0
    for i, ch in enumerate(s):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def fold(name, n):
    if not n or not name.endswith(">"):
        return name
    cut = name.index("<")                              # the outermost argument list, split at its top-level commas
    head, args = name[:cut], name[cut + 1:-1]
    parts, depth, cur = [], 0, ""
    for ch in args:
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "," and depth == 0:
            parts.append(cur.strip()); cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    if len(parts) < n or any(p not in ("true", "false") for p in parts[-n:]):
        return name
    mask = sum((p == "true") << k for k, p in enumerate(parts[-n:]))
    return f"{head}<{', '.join(parts[:-n] + [str(mask) + 'u'])}>"


def load(path, nfold, no_block_names=False):
    lines = open(path).read().split("\n")
    if no_block_names:
        lines = [re.sub(r"(^; %bb\.\d+:|:)\s*; %\S+$", r"\1", ln) for ln in lines]
    label = {ln.split(":", 1)[0]: i for i, ln in enumerate(lines) if re.match(r"[A-Za-z_][\w$.]*:", ln)}   # `symbol:   ; @symbol`
    syms = [ln.split()[1] for ln in lines if ln.startswith("\t.amdhsa_kernel ")]
    dem = demangle(syms)
    local = re.compile(r"(\.LBB|\.Lfunc_begin|\.Lfunc_end|\.Ltmp|\bBB)\d+")      # (BB12_3: the same labels inside the compiler's loop comments)
    pad = re.compile(r"\s+;")                                # (a label's comment column moves with the digits of its index)
    kernels = {}
    desc = {ln.split()[1]: i for i, ln in enumerate(lines) if ln.startswith("\t.amdhsa_kernel ")}
    for sym in syms:
        i = j = label[sym]
        while not lines[j].startswith(".Lfunc_end"):       # the function: entry label .. end label
            j += 1
        d = e = desc[sym]
        while lines[e].strip() != ".end_amdhsa_kernel":    # the kernel descriptor (wherever the compiler put it)
            e += 1
        info = [ln for ln in lines[e:e + 60] if ln.startswith("; Occupancy:")][:1]
        kernels[fold(short(dem[sym]), nfold)] = [pad.sub(" ;", local.sub(r"\1", ln.replace(sym, "<self>"))) for ln in lines[i:j + 1] + lines[d:e + 1] + info]
    m = lines.index("amdhsa.kernels:")
    entry = []
    for ln in lines[m + 1:]:
        if ln.startswith("  - ") or not ln.startswith("  "):     # the next kernel's entry, or the end of the list
            if entry:
                sym = next(x.split()[1] for x in entry if x.lstrip().startswith(".name:"))
                kernels[fold(short(dem[sym]), nfold)] += ["; metadata"] + [x.replace(sym, "<self>") for x in entry]
            entry = []
            if not ln.startswith("  "):
                break
        entry.append(ln)
    return kernels


def load_side(spec, nfold, no_block_names=False):
    """The merged kernels of one side: a file, files joined by commas, or a directory of .s files."""
    paths = sorted(glob.glob(os.path.join(spec, "*.s"))) if os.path.isdir(spec) else spec.split(",")
    if not paths:
        sys.exit(f"no .s file in {spec}")
    merged, origin = {}, {}
    for p in paths:
        for k, text in load(p, nfold, no_block_names).items():
            if k in merged:
                print(f"error: kernel compiled twice on one side: {k}\n  in {origin[k]}\n  and {p}")
                sys.exit(2)
            merged[k], origin[k] = text, p
    return merged


def numbers(text):
    meta = text[text.index("; metadata"):]
    got = {k: next((x.split()[-1] for x in meta if x.strip(" -").startswith("." + k + ":")), "?") for k in RES}
    got["occupancy"] = next((x.split()[-1] for x in text if x.startswith("; Occupancy:")), "?")
    return got


def resources(text):
    return " ".join(f"{k}={v}" for k, v in numbers(text).items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("a", help="one .s file, several joined by commas, or a directory of them")
    ap.add_argument("b", help="the same for the other side")
    ap.add_argument("--fold-bools", type=int, default=0, metavar="N")
    ap.add_argument("--list-same", action="store_true", help="also list the kernels that are identical, with their resource numbers")
    ap.add_argument("--no-block-names", action="store_true", help="ignore the IR block names in label comments (names of inlined functions)")
    ap.add_argument("--brief", action="store_true", help="one line per differing kernel; --list-same counts the identical ones per kernel name")
    a = ap.parse_args()
    A, B = load_side(a.a, a.fold_bools, a.no_block_names), load_side(a.b, 0, a.no_block_names)
    both = sorted(set(A) & set(B))
    same = [k for k in both if A[k] == B[k]]
    diff = [k for k in both if A[k] != B[k]]
    print(f"kernels: {len(A)} in A, {len(B)} in B, {len(both)} matched by name, {len(same)} identical (instructions, descriptor, metadata), {len(diff)} different")
    for tag, only in (("A", sorted(set(A) - set(B))), ("B", sorted(set(B) - set(A)))):
        for k in only:
            print(f"only in {tag}: {k}")
    if a.brief:
        moved = {k: " ".join(f"{r}={x}>{y}" for (r, x), y in zip(numbers(A[k]).items(), numbers(B[k]).values()) if x != y) for k in diff}
        for k in diff:
            if moved[k]:
                print(f"different: {k} | {moved[k]}")
        names = [k.split("<")[0] for k in diff if not moved[k]]
        for k in sorted(set(names)):
            print(f"different, every resource number equal: {names.count(k)} x {k}")
    for k in () if a.brief else diff:
        at = next((i for i, (x, y) in enumerate(zip(A[k], B[k])) if x != y), min(len(A[k]), len(B[k])))
        print(f"different: {k}\n  A: {resources(A[k])}\n  B: {resources(B[k])}\n  first difference at line {at} of {len(A[k])} / {len(B[k])}:"
              f"\n  A| {A[k][at] if at < len(A[k]) else '<end>'}\n  B| {B[k][at] if at < len(B[k]) else '<end>'}")
    if a.list_same and a.brief:
        names = [k.split("<")[0] for k in same]
        for k in sorted(set(names)):
            print(f"identical: {names.count(k)} x {k}")
    elif a.list_same:
        for k in same:
            print(f"identical: {k} | {resources(A[k])}")
    sys.exit(0 if len(same) == len(A) == len(B) else 1)
