"""The library's source list (build.SOURCES) against the tree: every .hip is built, every .hpp is included from a built source, and
every function of the public header is defined in exactly one source.  Reads text only: compiles nothing, needs no GPU."""
import os
import re

from rl_aerial_manipulator_amd.build import CSRC, SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(path):
    with open(path) as f:
        return f.read()


def test_every_hip_source_is_built():
    on_disk = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert on_disk == sorted(SOURCES), "csrc/*.hip and build.SOURCES differ"
    assert len(set(SOURCES)) == len(SOURCES)


def test_every_header_is_reachable_from_a_source():
    seen, todo = set(), list(SOURCES)
    while todo:
        name = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _read(os.path.join(CSRC, name)), re.M):
            inc = os.path.normpath(inc)
            if not inc.startswith("..") and inc not in seen:   # (../../include/amenv.h: outside csrc/)
                assert os.path.exists(os.path.join(CSRC, inc)), f"{name} includes {inc}, which is not in csrc/"
                seen.add(inc)
                todo.append(inc)
    headers = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp"))
    assert [h for h in headers if h not in seen] == [], "headers that no source of build.SOURCES includes"


def test_every_public_function_is_defined_in_exactly_one_source():
    header = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "amenv.h")), flags=re.S)
    header = re.sub(r"//[^\n]*", "", header)
    declared = sorted(set(re.findall(r"\b(amenv_\w+)\s*\(", header)))
    assert {"amenv_version", "amenv_create", "amenv_step", "amenv_rollout_policy_norm", "amenv_ppo_mlp_step", "amenv_pid_policy"} <= set(declared), \
        "the public header's declarations were not found"
    text = {s: _read(os.path.join(CSRC, s)) for s in SOURCES}
    for name in declared:
        # a definition starts in column 0 with the return type: `int NAME(`, `const char* NAME(`, `size_t NAME(`, `int64_t NAME(`, ...
        pat = re.compile(r"^(?:const\s+)?\w+\s*\*?\s*" + name + r"\(", re.M)
        holders = [s for s, t in text.items() for _ in pat.findall(t)]
        assert len(holders) == 1, f"{name} is defined {len(holders)} times: {holders}"
