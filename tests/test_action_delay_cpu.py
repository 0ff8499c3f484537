"""Per-episode actuation latency, host side (no GPU; include/amenv.h amenv_set_action_delay): ActionDelay's checks
and C layout, the three declared and exported entry points, the d draw restated in tests/delay_ref.py, and the reference checkpoint flown
on the delayed oracle (the reference side of the GPU test of how a policy flies)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from oracle import oracle as O
from rl_aerial_manipulator_amd.ppo import ActorCritic
from tests import delay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- 1. ActionDelay, the C layout, the symbols -----------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(-1,), (9,), (3, 2), (0, 9), (-1, 4), (1.5,), (0, 2.0), ("2",), (True,), (0, False), (None,), ((1, 2),)])
def test_range_is_checked(args):
    with pytest.raises(amd.AmenvError):
        amd.ActionDelay(*args)


def test_action_delay_accepted_and_packed():
    z = amd.ActionDelay(3)
    assert (z.min_steps, z.max_steps) == (3, 3) and repr(z) == "ActionDelay(3, 3)"
    z = amd.ActionDelay(np.int32(0), np.int64(8))
    assert (z.min_steps, z.max_steps) == (0, 8) and repr(z) == "ActionDelay(0, 8)"
    assert amd.ActionDelay(0).max_steps == 0
    c = amd.ActionDelay(2, 5)._as_c()
    assert C.sizeof(c) == 12 and c.struct_size == 12 and (c.min_steps, c.max_steps) == (2, 5)
    assert [f[0] for f in amd._lib.ActionDelayC._fields_] == ["struct_size", "min_steps", "max_steps"]
    assert amd._lib.ActionDelayC.min_steps.offset == 4 and amd._lib.ActionDelayC.max_steps.offset == 8
    assert amd._lib.MAX_ACTION_DELAY == 8 == delay_ref.MAX_DELAY


def test_env_refuses_a_bad_delay_before_any_device_is_touched():
    with pytest.raises(amd.AmenvError):
        amd.GpuWaypointEnv(8, action_delay=amd.ActionDelay(9))
    with pytest.raises(amd.AmenvError, match="ActionDelay"):
        amd.GpuWaypointEnv(8, action_delay=2)


def test_action_delay_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "amenv.h")).read()
    lib = C.CDLL(amd._lib.LIB_PATH)
    for name in ("amenv_set_action_delay", "amenv_get_action_delay_state", "amenv_set_action_delay_state"):
        assert name + "(" in hdr, name
        assert name in amd._lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct amenv_action_delay" in hdr and "AMENV_ABI_VERSION 2" in hdr and "#define AMENV_MAX_ACTION_DELAY 8" in hdr
    assert "ActionDelay" in amd.__all__


# ---- 2. the d draw ---------------------------------------------------------------------------------------------------------------
def test_draw_covers_the_range_evenly():
    """gids 0..4095, episodes 1..4, range 0..8: 16,384 draws, every value within 0.85x .. 1.15x of 16384 / 9 (a binomial count there has a
    standard deviation of 40 = 2.2 %: the bound is about 6.8 sigma)."""
    d = np.array([delay_ref.draw(5, g, ep, 0, 8) for ep in range(1, 5) for g in range(4096)])
    counts = np.bincount(d, minlength=9)
    print("d counts 0..8:", counts.tolist())
    assert len(counts) == 9 and d.min() == 0 and d.max() == 8
    mean = 16384 / 9
    assert np.all(counts >= 0.85 * mean) and np.all(counts <= 1.15 * mean), counts


def test_draw_of_a_fixed_range_is_that_value_and_depends_on_every_key_part():
    for lo in (0, 3, 8):
        assert all(delay_ref.draw(7, g, ep, lo, lo) == lo for g in range(64) for ep in (1, 2))
    assert np.array_equal(delay_ref.draw_all(7, 100, [1, 1, 2], 2, 6), [delay_ref.draw(7, 100, 1, 2, 6), delay_ref.draw(7, 101, 1, 2, 6), delay_ref.draw(7, 102, 2, 2, 6)])
    base = [delay_ref.draw(7, g, 1, 0, 8) for g in range(256)]
    assert base != [delay_ref.draw(8, g, 1, 0, 8) for g in range(256)]          # seed
    assert base != [delay_ref.draw(7, g, 2, 0, 8) for g in range(256)]          # episode
    assert base != [delay_ref.draw(7, g + (1 << 32), 1, 0, 8) for g in range(256)]   # the id's high word
    assert all(2 <= delay_ref.draw(7, g, 1, 2, 6) <= 6 for g in range(256))


def test_history_is_in_age_order_and_refills_with_hover():
    h = delay_ref.History(3, 0, [1, 1], 2, 2)
    rows = np.arange(40, dtype=np.float32).reshape(5, 2, 4)
    assert np.array_equal(h.applied(rows[0]), np.tile(delay_ref.HOVER, (2, 1)))
    h.push(rows[0]); assert np.array_equal(h.applied(rows[1]), np.tile(delay_ref.HOVER, (2, 1)))
    h.push(rows[1]); assert np.array_equal(h.applied(rows[2]), rows[0])
    h.push(rows[2], np.array([True, False]), [2, 1])
    assert np.array_equal(h.recent[0], np.tile(delay_ref.HOVER, (8, 1))) and np.array_equal(h.recent[1, :3], rows[[2, 1, 0], 1])
    assert np.array_equal(h.applied(rows[3]), np.stack([delay_ref.HOVER, rows[1, 1]]))
    z = delay_ref.History(3, 0, [1, 1], 0, 0)
    assert np.array_equal(z.applied(rows[4]), rows[4])


# ---- 3. the reference checkpoint on the delayed oracle ---------------------------------------------------------------------------
def _fly(d, n=64, steps=1400):
    z = np.load(os.path.join(GOLD, "policy_2300000.npz"))
    pol = ActorCritic.from_sb3({k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("_")})
    orc = delay_ref.DelayedOracle(O.reference_quad_config(num_envs=n, seed=5), d)
    obs = orc.reset()
    episodes = success = crashed = 0
    for _ in range(steps):
        out = orc.step(pol.predict(torch.from_numpy(obs)).numpy())
        obs, done, info = out["obs"], out["done"], out["info"]
        episodes += int(done.sum())
        success += int(((done != 0) & ((info & 4) != 0)).sum())       # episodes that ended with AMENV_INFO_SUCCESS
        crashed += int(((done != 0) & ((info & 16) != 0)).sum())      # ... with AMENV_INFO_CRASHED
    return episodes, success, crashed


def test_reference_checkpoint_tolerates_ten_milliseconds_on_the_oracle():
    episodes, success, crashed = _fly(2)
    print("d = 2:", episodes, success, crashed)
    assert episodes >= 64 and success >= 0.90 * episodes, (episodes, success, crashed)


def test_reference_checkpoint_falls_apart_at_forty_milliseconds_on_the_oracle():
    episodes, success, crashed = _fly(8)
    print("d = 8:", episodes, success, crashed)
    assert episodes >= 64 and success < 0.10 * episodes and crashed > 0.5 * episodes, (episodes, success, crashed)
