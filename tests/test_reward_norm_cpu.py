"""CPU-only checks of the reward normaliser: the C ABI refuses bad arguments before it looks for a device and fails loudly without
one, the numpy reference has the chunking property the GPU design rests on, and statistics files written before the return statistics
existed still load."""
import ctypes as C

import numpy as np
import pytest

import rl_aerial_manipulator_amd as amd
from tests import retnorm_ref as R


def test_retnorm_create_refuses_bad_arguments_and_fails_loudly_without_a_device():
    import torch
    L = amd._lib.load()
    h = C.c_void_p()
    for n, gamma in ((0, 0.99), (-5, 0.99), (64, -0.1), (64, 1.5), (64, float("nan")), (64, float("inf"))):
        assert L.amenv_retnorm_create(n, gamma, 0, C.byref(h)) == -1, (n, gamma)
        assert b"amenv_retnorm_create" in L.amenv_last_error(None)
    assert L.amenv_retnorm_create(64, 0.99, 0, None) == -1
    assert L.amenv_retnorm_create(64, 0.99, 10 ** 6, C.byref(h)) == -3        # no such device, with or without a GPU
    rc = L.amenv_retnorm_create(64, 0.99, 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and L.amenv_retnorm_destroy(h) == 0
    else:
        assert rc == -3 and b"no such HIP device" in L.amenv_last_error(None)
        with pytest.raises(amd.AmenvError, match="amenv_retnorm_create failed"):
            amd.RewardNormalizer(64)
    # NULL handle / buffers and n_steps <= 0 are refused before any launch
    assert L.amenv_retnorm_rollout(None, 1, None, None, None, 1, 10.0, 1e-8, None) == -1
    assert L.amenv_retnorm_reset_returns(None, None) == -1 and L.amenv_retnorm_get(None, None, None, None, None, None) == -1
    assert L.amenv_retnorm_set(None, 0.0, 1.0, 1.0, None, None) == -1 and L.amenv_retnorm_destroy(None) == 0


@pytest.mark.parametrize("N,T", [(1, 7), (65, 130), (257, 33)])
def test_reference_one_step_calls_equal_one_block_call(N, T):
    r, d = R.make_block(T, N, seed=N * 1000 + T)
    a, b, c = R.RetNormRef(N), R.RetNormRef(N), R.RetNormRef(N)
    one = a.block(r, d)
    steps = np.concatenate([b.block(r[t:t + 1], d[t:t + 1]) for t in range(T)])
    cut = max(1, T // 2)
    split = np.concatenate([c.block(r[:cut], d[:cut]), c.block(r[cut:], d[cut:])]) if cut < T else c.block(r, d)
    assert np.array_equal(one, steps) and np.array_equal(one, split)
    for x, y, z in zip(a.state(), b.state(), c.state()):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert abs(a.count - (1e-4 + T * N)) < 1e-6 and np.isfinite(one).all() and np.abs(one).max() <= 10.0
    # frozen: the state does not move and every row is scaled with the entry variance
    before = a.state()
    f = a.block(r, d, update=False)
    assert all(np.array_equal(x, y) for x, y in zip(before, a.state()))
    assert np.array_equal(f, np.clip(r.astype(np.float64) / np.sqrt(a.var + 1e-8), -10, 10))


class _StubNormalizer:
    def set(self, mean, var, count):
        self.args = (np.asarray(mean), np.asarray(var), float(count))

    def close(self):
        pass


class _StubVenv:
    num_envs = 8

    class observation_space:
        shape = (17,)

    action_space = None


def test_statistics_file_without_return_statistics_loads_with_norm_reward_off(tmp_path):
    """An .npz as GpuVecNormalize.save wrote it before norm_reward existed: the five observation-statistics members only."""
    mean, var = np.arange(17.0), np.arange(17.0) + 1.0
    np.savez(str(tmp_path / "old.npz"), mean=mean, var=var, count=123.0, clip_obs=5.0, epsilon=1e-6)
    stub = _StubNormalizer()
    env = amd.GpuVecNormalize.load(str(tmp_path / "old"), _StubVenv(), normalizer=stub)
    assert env.norm_reward is False and env.ret_rms is None and env.norm_obs is True
    assert env.clip_obs == 5.0 and env.epsilon == 1e-6
    assert np.array_equal(stub.args[0], mean) and np.array_equal(stub.args[1], var) and stub.args[2] == 123.0
    r = np.array([1.0, -2.0], np.float32)
    assert env.normalize_reward(r) is r and env.get_original_reward() is None
