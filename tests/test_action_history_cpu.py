"""Action history in the observation rows, host side (no GPU; include/amenv.h amenv_set_action_history):
ActionHistory's checks, the two declared and exported entry points, the MLP shapes the wider rows need, and tests/history_ref.py against
a hand-written example."""
import ctypes as C
import os

import numpy as np
import pytest

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd.ppo import ActorCritic
from tests import delay_ref, history_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows", [0, 3, -1, 1.0, 2.5, "2", True, None, (1,)])
def test_rows_are_checked(rows):
    with pytest.raises(amd.AmenvError, match="ActionHistory"):
        amd.ActionHistory(rows)


def test_action_history_accepted():
    assert amd.ActionHistory(1).rows == 1 and amd.ActionHistory(2).rows == 2
    assert amd.ActionHistory(np.int64(2)).rows == 2 and repr(amd.ActionHistory(np.int32(1))) == "ActionHistory(1)"
    assert "ActionHistory" in amd.__all__


def test_env_refuses_a_bad_history_before_any_device_is_touched():
    with pytest.raises(amd.AmenvError):
        amd.GpuWaypointEnv(8, action_history=amd.ActionHistory(3))
    with pytest.raises(amd.AmenvError, match="ActionHistory"):
        amd.GpuWaypointEnv(8, action_history=2)


def test_action_history_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "amenv.h")).read()
    lib = C.CDLL(amd._lib.LIB_PATH)
    for name in ("amenv_set_action_history", "amenv_obs_dim"):
        assert name + "(" in hdr, name
        assert name in amd._lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "int amenv_set_action_history(amenv* env, int32_t rows);" in hdr and "int32_t amenv_obs_dim(const amenv* env);" in hdr
    assert "AMENV_ABI_VERSION 2" in hdr


def test_mlp_shapes_of_the_wider_rows():
    new = {(24, 4), (28, 4), (21, 4), (25, 4)}
    assert new <= ActorCritic._FUSED_DIMS and {(20, 4), (29, 7), (17, 4), (25, 5), (27, 6)} <= ActorCritic._FUSED_DIMS
    for D, A in sorted(new):   # amenv_team_policy.hpp PolLayout: log_std | pi trunk | vf trunk | head W, b | value W, b
        trunk = 128 * D + 128 + 64 * 128 + 64 + 64 * 64 + 64
        assert ActorCritic(D, A).flatten_().flat_param.numel() == A + 2 * trunk + 64 * A + A + 64 + 1, (D, A)


def test_history_ref_on_a_hand_written_example():
    """Two envs, six steps, env 0 resets after step 3 (its fourth).  Rows are (10 t + env, 0, 0, t)."""
    H = delay_ref.HOVER
    a = np.zeros((6, 2, 4), np.float32)
    for t in range(6):
        for i in range(2):
            a[t, i] = (10 * t + i, 0, 0, t)
    hist = delay_ref.History(3, 0, [1, 1], 0, 0)
    assert np.array_equal(history_ref.rows(hist, 2), np.tile(np.concatenate([H, H]), (2, 1)))
    assert history_ref.rows(hist, 1).shape == (2, 4) and history_ref.rows(hist, 1).dtype == np.float32
    expect_step = {   # (t, env) -> the 8 columns of the row published after step t
        (0, 0): np.concatenate([a[0, 0], H]), (0, 1): np.concatenate([a[0, 1], H]),
        (1, 0): np.concatenate([a[1, 0], a[0, 0]]), (1, 1): np.concatenate([a[1, 1], a[0, 1]]),
        (2, 0): np.concatenate([a[2, 0], a[1, 0]]), (2, 1): np.concatenate([a[2, 1], a[1, 1]]),
        (3, 0): np.concatenate([H, H]),             (3, 1): np.concatenate([a[3, 1], a[2, 1]]),     # env 0: the new episode's row
        (4, 0): np.concatenate([a[4, 0], H]),       (4, 1): np.concatenate([a[4, 1], a[3, 1]]),
        (5, 0): np.concatenate([a[5, 0], a[4, 0]]), (5, 1): np.concatenate([a[5, 1], a[4, 1]])}
    for t in range(6):
        term = history_ref.pushed(hist, a[t], 2)
        reset = np.array([t == 3, False])
        hist.push(a[t], reset, [2, 1])
        got = history_ref.rows(hist, 2)
        for i in range(2):
            assert np.array_equal(got[i], expect_step[(t, i)]), (t, i)
            assert np.array_equal(history_ref.rows(hist, 1)[i], expect_step[(t, i)][:4]), (t, i)
        if t == 3:   # the terminal row of env 0 ends in [a_3, a_2]: the history before the refill
            assert np.array_equal(term[0], np.concatenate([a[3, 0], a[2, 0]]))
            assert np.array_equal(history_ref.pushed(delay_ref.History(3, 0, [1, 1], 0, 0), a[0], 1)[0], a[0, 0])
        assert np.array_equal(term[1], expect_step[(t, 1)])   # an env that goes on: the terminal columns are the step row's


def test_history_oracle_appends_to_the_oracle_rows():
    from oracle import oracle as O
    n = 8
    cfg = O.reference_quad_config(num_envs=n, seed=5)
    cfg.task.max_episode_steps = 4
    orc = history_ref.HistoryOracle(cfg, 2)
    o0 = orc.reset()
    assert o0.shape == (n, 28) and np.array_equal(o0[:, 20:], np.tile(np.concatenate([delay_ref.HOVER] * 2), (n, 1)))
    rng = np.random.RandomState(0)
    prev = np.tile(delay_ref.HOVER, (n, 1))
    saw_reset = False
    for t in range(9):
        a = rng.uniform([0.8, -0.1, -0.1, -0.1], [1.2, 0.1, 0.1, 0.1], size=(n, 4)).astype(np.float32)
        out = orc.step(a)
        reset = (out["info"] & delay_ref.WAS_RESET) != 0
        saw_reset |= bool(reset.any())
        assert np.array_equal(out["terminal_hist"], np.concatenate([a, prev], axis=1))
        assert np.array_equal(out["obs"][~reset, 20:], np.concatenate([a, prev], axis=1)[~reset])
        assert np.array_equal(out["obs"][reset, 20:], np.tile(np.concatenate([delay_ref.HOVER] * 2), (int(reset.sum()), 1)))
        assert np.all(orc.hist.d == 0)
        prev = np.where(reset[:, None], delay_ref.HOVER, a)
    assert saw_reset
