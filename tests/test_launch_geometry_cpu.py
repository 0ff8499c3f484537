"""The sizes of tests/test_gpu_launch_geometry.py only cross the launchers' thresholds while the caps stay where they are: this test reads
the constants and launcher expressions from csrc/ with plain regular expressions, recomputes every threshold of that module's GEOMETRY
table from them, and asserts that each has a tested size at or below it and one above it.  No GPU and no build needed."""
import os
import re

from rl_aerial_manipulator_amd.build import SOURCES
from tests.test_gpu_launch_geometry import GEOMETRY

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-aerial-manipulator_amd", "csrc")
HINT = "update the row of GEOMETRY in tests/test_gpu_launch_geometry.py (threshold and the sizes that straddle it)"


def _read(csrc, name):
    with open(os.path.join(csrc, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)\b", text)
    assert m, f"constant {name} not found"
    return int(m.group(1))


def _body(text, func):
    """Source of the C-ABI function `func`: from its definition to the closing brace in column 0."""
    m = re.search(r"^int " + func + r"\(.*?^}", text, re.S | re.M)
    assert m, f"launcher {func} not found"
    return m.group(0)


def _int(body, pattern, what):
    m = re.search(pattern, body)
    assert m, f"{what}: expression not found (the launcher changed: re-derive the thresholds, then {HINT})"
    return [int(g) for g in m.groups()]


def thresholds_from_sources(csrc=CSRC):
    """{row: threshold} of every GEOMETRY row, from the sources under `csrc`."""
    train, mlp = _read(csrc, "amenv_train.hpp"), _read(csrc, "amenv_mlp_train.hpp")
    capi = "\n".join(_read(csrc, s) for s in SOURCES)   # the C-ABI entry points, whichever source holds them
    ppo_block, ppo_max = _const(train, "kPpoBlock"), _const(train, "kPpoMaxBlocks")
    adam_block, adam_max = _const(mlp, "kAdamBlock"), _const(mlp, "kAdamMaxBlocks")
    red_groups, mlp_max = _const(mlp, "kRedGroups"), _const(mlp, "kMlpMaxBlocks")
    t = {}
    # amenv_policy_forward_mfma: grid.x = min(512 / nets, ceil(tiles / 4)), 32 rows per tile
    b = _body(capi, "amenv_policy_forward_mfma")
    (rows,) = _int(b, r"ntiles = \(n \+ \d+\) / (\d+);", "forward_mfma rows per tile")
    cap, tiles = _int(b, r"std::min<int64_t>\((\d+) / nets, \(ntiles \+ \d+\) / (\d+)\)", "forward_mfma grid")
    t["fwd_mfma_both"] = cap // 2 * tiles * rows
    t["fwd_mfma_both_round2"] = 2 * t["fwd_mfma_both"]
    t["fwd_mfma_one"] = cap * tiles * rows
    (t["fwd_valu_block"],) = _int(_body(capi, "amenv_policy_forward"), r"\(n \+ \d+\) / (\d+)\), 2\)", "policy_forward grid")
    # amenv_ppo_loss_grad: min(kPpoMaxBlocks, ceil(n / kPpoBlock)) workgroups
    b = _body(capi, "amenv_ppo_loss_grad")
    assert re.search(r"std::min<int64_t>\(kPpoMaxBlocks, \(n \+ kPpoBlock - 1\) / kPpoBlock\)", b), f"loss grid changed: {HINT}"
    t["loss_block"], t["loss_round"], t["loss_round2"] = ppo_block, ppo_max * ppo_block, 2 * ppo_max * ppo_block
    # amenv_ppo_mlp_step: min(128, ceil(tiles / 4)) workgroups of 4 tiles x 32 samples; advantage partials as the loss kernel
    b = _body(capi, "amenv_ppo_mlp_step")
    (rows,) = _int(b, r"ntiles = \(n \+ \d+\) / (\d+);", "mlp_step rows per tile")
    cap, tiles = _int(b, r"blocks = int\(std::min<int64_t>\((\d+), \(ntiles \+ \d+\) / (\d+)\)\)", "mlp_step grid")
    assert cap <= mlp_max, "more slabs than the workspace holds"
    assert re.search(r"adv_blocks = int\(std::min<int64_t>\(kPpoMaxBlocks, \(n \+ kPpoBlock - 1\) / kPpoBlock\)\)", b), f"mlp_step advantage grid changed: {HINT}"
    t["step_slab"] = tiles * rows
    t["step_reduce_groups"] = red_groups * tiles * rows
    t["step_round"] = cap * tiles * rows
    t["step_adv_round"] = t["step_adv_round_gather"] = ppo_max * ppo_block
    # amenv_ppo_adam_step: min(kAdamMaxBlocks, ceil(n / kAdamBlock)) workgroups; float4 norm pass over n >> 2 vectors
    b = _body(capi, "amenv_ppo_adam_step")
    assert re.search(r"std::min<int64_t>\(kAdamMaxBlocks, \(n \+ kAdamBlock - 1\) / kAdamBlock\)", b), f"Adam grid changed: {HINT}"
    assert re.search(r"n4 = n >> 2;", mlp), f"Adam norm pass changed: {HINT}"
    t["adam_float4"], t["adam_block"], t["adam_grid"] = 3, adam_block, adam_max * adam_block
    # amenv_gae / amenv_gaussian_act: 64 lanes up to 65536 envs, 256 beyond
    for row, func in (("gae_block", "amenv_gae"), ("act_block", "amenv_gaussian_act")):
        t[row], small, large = _int(_body(capi, func), r"bs = n_envs <= (\d+) \? (\d+) : (\d+);", func + " block size")
        assert small != large
    # amenv_obsnorm_*: 256-thread workgroups, 1024 (update) / 2048 (apply) of them; at the widest arm observation (29 floats per row)
    for row, func in (("obsnorm_update_grid", "amenv_obsnorm_update"), ("obsnorm_apply_grid", "amenv_obsnorm_apply")):
        b = _body(capi, func)
        (bs,) = _int(b, r"bs = (\d+);", func + " block size")
        cap, cap2 = _int(b, r"if \(blocks > (\d+)\) blocks = (\d+);", func + " grid cap")
        assert cap == cap2
        t[row] = cap * bs // 29
        if func == "amenv_obsnorm_update":
            t["obsnorm_block_dim"] = bs
    (t["obsnorm_max_dim"],) = _int(_body(capi, "amenv_obsnorm_create"), r"dim <= 0 \|\| dim > (\d+)", "obsnorm_create largest dim")
    return t


def test_every_threshold_is_recomputed_from_the_sources_and_straddled():
    derived = thresholds_from_sources()
    rows = [r[0] for r in GEOMETRY]
    assert len(set(rows)) == len(rows) and set(rows) == set(derived), (sorted(set(rows) ^ set(derived)), HINT)
    for row, kernel, what, threshold, sizes in GEOMETRY:
        assert derived[row] == threshold, f"{row} ({kernel}: {what}): the sources give {derived[row]}, the table says {threshold}: {HINT}"
        assert any(s <= threshold for s in sizes), f"{row} ({kernel}): no tested size at or below {threshold}: {HINT}"
        assert any(s > threshold for s in sizes), f"{row} ({kernel}): no tested size above {threshold}: {HINT}"
