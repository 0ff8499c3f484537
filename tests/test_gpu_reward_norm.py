"""GPU reward normaliser (amenv_retnorm_*, RewardNormalizer, GpuVecNormalize(norm_reward=True), PPO(reward_normalizer=...)) against the
fp64 numpy restatement of SB3 2.6.0's VecNormalize reward path in tests/retnorm_ref.py (third-party semantics, parity unpinned).

Tolerances: mean rtol 1e-9, var rtol 1e-8 and outputs rtol = atol = 2e-6 are those of tests/test_gpu_obsnorm.py (fp64 statistics whose
reduction order differs from numpy's, one fp32 rounding of the output); the count is a sum of the same fp64 additions and must be exact;
the carried returns are the same fp64 multiply-add per env and are held to the project's fp64 gate of 1e-12 relative."""
import functools
import io
import zipfile

import numpy as np
import pytest

from tests import retnorm_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 257, 1000)      # one lane | a wave minus one | exactly one | one plus a lane | 5 waves, ragged | 16 waves, ragged
TS = (1, 2, 7, 130)                  # 130 crosses the 128-step workspace chunk


@functools.lru_cache(maxsize=None)
def case(T, N):
    """Inputs and the reference's answer for a fresh normaliser, computed once per shape and never modified."""
    r, d = R.make_block(T, N, seed=7919 * N + T)
    ref = R.RetNormRef(N)
    out = ref.block(r, d)
    for a in (r, d, out):
        a.setflags(write=False)
    return r, d, out, ref.state()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the cached inputs are read-only


def state_bytes(nz):
    m, v, c, ret = nz.get()
    return np.array([m, v, c]).tobytes() + ret.tobytes()


def check_outputs(got, want):
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_training_block_matches_the_reference(T, N):
    import rl_aerial_manipulator_amd as amd
    r, d, want, (mean, var, count, returns) = case(T, N)
    nz = amd.RewardNormalizer(N)
    got = nz.normalize(dev(r), dev(d)).cpu().numpy()
    gm, gv, gc, gret = nz.get()
    nz.close()
    assert gc == count
    np.testing.assert_allclose(gm, mean, rtol=1e-9)
    np.testing.assert_allclose(gv, var, rtol=1e-8)
    assert np.all(np.abs(gret - returns) <= 1e-12 * np.abs(returns))
    check_outputs(got, want)
    assert np.abs(got).max() <= 10.0


@pytest.mark.parametrize("N", NS)
def test_chunking_is_invisible_bit_for_bit(N):
    """One call of 130 steps, 130 calls of one step, and calls of 64, 1 and 65 steps: identical outputs, statistics and returns."""
    import rl_aerial_manipulator_amd as amd
    T = 130
    r, d, _, _ = case(T, N)
    rd, dd = dev(r), dev(d)
    results = []
    for cuts in ((0, 130), tuple(range(131)), (0, 64, 65, 130)):
        nz = amd.RewardNormalizer(N)
        out = np.concatenate([nz.normalize(rd[a:b], dd[a:b]).cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])])
        results.append((out.tobytes(), state_bytes(nz)))
        nz.close()
    assert results[0] == results[1] and results[0] == results[2]


@pytest.mark.parametrize("T,N", [(130, 1000), (7, 65)])
def test_two_runs_from_the_same_state_are_identical(T, N):
    import rl_aerial_manipulator_amd as amd
    r, d, _, _ = case(T, N)
    nz = amd.RewardNormalizer(N)
    nz.normalize(dev(r), dev(d))
    start = nz.get()
    runs = []
    for _ in range(2):
        nz.set(*start)
        runs.append((nz.normalize(dev(r), dev(d)).cpu().numpy().tobytes(), state_bytes(nz)))
    nz.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_frozen_mode_scales_with_the_entry_variance_and_changes_nothing(T, N):
    import rl_aerial_manipulator_amd as amd
    r, d, _, (_, var, _, _) = case(T, N)
    nz = amd.RewardNormalizer(N)
    nz.normalize(dev(r), dev(d))                     # some statistics and non-zero returns to freeze
    before = state_bytes(nz)
    r2 = (r[::-1] * np.float32(0.5)).copy()
    got = nz.normalize(dev(r2), dev(d), update=False).cpu().numpy()
    no_dones = nz.normalize(dev(r2), None, update=False).cpu().numpy()
    assert state_bytes(nz) == before
    nz.close()
    check_outputs(got, np.clip(r2.astype(np.float64) / np.sqrt(var + 1e-8), -10, 10))
    assert np.array_equal(got, no_dones)


@pytest.mark.parametrize("T,N", [(130, 257), (2, 63), (1, 1)])
def test_in_place_and_clipping(T, N):
    import torch
    import rl_aerial_manipulator_amd as amd
    r, d, _, _ = case(T, N)
    a, b = amd.RewardNormalizer(N), amd.RewardNormalizer(N)
    out = a.normalize(dev(r), dev(d))
    buf = dev(r)
    assert b.normalize(buf, dev(d), out=buf) is buf
    assert torch.equal(out, buf) and state_bytes(a) == state_bytes(b)
    # |r / sigma| > clip: exactly +-clip, frozen (sigma = 1, |r| ~ 1e6) and training (|r| >= ~100, sigma stays of order 1 to 10, clip 0.25)
    sign = np.where(np.arange(T * N).reshape(T, N) % 3 == 0, -1.0, 1.0)
    big = (sign * (1e6 + 1e3 * (np.arange(T * N).reshape(T, N) % 7))).astype(np.float32)
    b.set(0.0, 1.0, 1e6, np.zeros(N))
    frozen = b.normalize(dev(big), None, update=False).cpu().numpy()
    assert np.array_equal(frozen, (10.0 * sign).astype(np.float32))
    c = amd.RewardNormalizer(N, clip_reward=0.25)
    c.set(0.0, 1.0, 1e12, np.zeros(N))               # a count this large pins the variance at 1 through the block
    trained = c.normalize(dev(r), dev(d)).cpu().numpy()
    assert np.array_equal(trained, np.where(r > 0, np.float32(0.25), np.float32(-0.25)))
    a.close(); b.close(); c.close()


def test_round_trips_and_reset_returns():
    import rl_aerial_manipulator_amd as amd
    T, N = 7, 257
    r, d, _, _ = case(T, N)
    r2, d2, _, _ = case(2, N)
    a = amd.RewardNormalizer(N, gamma=0.97, clip_reward=5.0, epsilon=1e-6)
    a.normalize(dev(r), dev(d))
    b = amd.RewardNormalizer(N, gamma=0.97, clip_reward=5.0, epsilon=1e-6)
    b.set(*a.get())
    c = amd.RewardNormalizer(N, gamma=0.97)
    sd = a.state_dict()
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in sd.values())
    f = io.BytesIO()
    np.savez(f, **sd)                                # plain arrays: storable without pickle
    z = np.load(io.BytesIO(f.getvalue()), allow_pickle=False)
    c.load_state_dict({k: z[k] for k in z.files})
    assert (c.clip_reward, c.epsilon) == (5.0, 1e-6)
    with pytest.raises(amd.AmenvError, match="gamma"):
        amd.RewardNormalizer(N, gamma=0.5).load_state_dict(sd)
    assert state_bytes(a) == state_bytes(b) == state_bytes(c)
    outs = [x.normalize(dev(r2), dev(d2)).cpu().numpy().tobytes() for x in (a, b, c)]
    assert outs[0] == outs[1] == outs[2] and state_bytes(a) == state_bytes(b) == state_bytes(c)
    m, v, cnt, ret = a.get()
    assert np.abs(ret).max() > 0
    a.reset_returns()
    m1, v1, cnt1, ret1 = a.get()
    assert (m1, v1, cnt1) == (m, v, cnt) and not ret1.any()
    with pytest.raises(amd.AmenvError):
        a.normalize(dev(r2)[:, :5], dev(d2)[:, :5])
    with pytest.raises(amd.AmenvError):
        a.set(0.0, -1.0, 1.0)
    a.close(); b.close(); c.close()


def test_vec_normalize_with_norm_reward(tmp_path):
    """GpuVecNormalize(GpuVecEnv(64), norm_reward=True): what an SB3 loop over VecNormalize(norm_reward=True) sees."""
    import rl_aerial_manipulator_amd as amd
    n = 64
    env = amd.GpuVecNormalize(amd.GpuVecEnv(num_envs=n, seed=3, max_episode_steps=25), norm_obs=True, norm_reward=True)
    env.reset()
    rng = np.random.RandomState(5)
    raw, dones, got = [], [], []
    for t in range(60):
        a = rng.uniform([0, -1, -1, -1], [2, 1, 1, 1], (n, 4)).astype(np.float32); a[:, 1:] *= 0.05
        _, rew, done, _ = env.step(a)
        raw.append(env.get_original_reward().copy()); dones.append(done.copy()); got.append(rew)
    raw, dones, got = np.stack(raw), np.stack(dones), np.stack(got)
    assert got.dtype == np.float32 and dones.sum() >= n and np.abs(raw - got).max() > 0
    ref = R.RetNormRef(n)
    check_outputs(got, ref.block(raw, dones))
    mean, var, count, returns = env.ret_rms.get()
    assert count == ref.count
    np.testing.assert_allclose(var, ref.var, rtol=1e-8)
    np.testing.assert_allclose(returns, ref.returns, rtol=1e-12, atol=0)
    probe = np.array([[1.0, -250.0, 1e9]], np.float32)
    np.testing.assert_allclose(env.normalize_reward(probe), np.clip(probe / np.sqrt(var + 1e-8), -10, 10), rtol=2e-6)
    env.save(str(tmp_path / "vn"))
    env2 = amd.GpuVecNormalize.load(str(tmp_path / "vn"), amd.GpuVecEnv(num_envs=n, seed=3, max_episode_steps=25))
    assert env2.norm_reward and (env2.clip_reward, env2.gamma) == (10.0, 0.99) and state_bytes(env2.ret_rms) == state_bytes(env.ret_rms)
    r2, d2, _, _ = case(2, n)
    assert env.ret_rms.normalize(dev(r2), dev(d2)).cpu().numpy().tobytes() == env2.ret_rms.normalize(dev(r2), dev(d2)).cpu().numpy().tobytes()
    assert state_bytes(env2.ret_rms) == state_bytes(env.ret_rms)
    env.training = False
    frozen = state_bytes(env.ret_rms)
    for t in range(3):
        _, rew, _, _ = env.step(a)
        check_outputs(rew, np.clip(env.get_original_reward().astype(np.float64) / np.sqrt(env.ret_rms.get()[1] + 1e-8), -10, 10))
    assert state_bytes(env.ret_rms) == frozen
    env.training = True
    env.reset()
    assert not env.ret_rms.get()[3].any() and env.ret_rms.get()[:3] == env2.ret_rms.get()[:3]   # reset(): the returns restart, the statistics stay
    env.close(); env2.close()


@pytest.mark.parametrize("fused", [False, True], ids=["step_by_step", "one_launch"])
def test_ppo_normalises_after_the_rollout_and_before_the_bootstrap(fused, tmp_path):
    """64 quadrotors, 40-step time limit, 96-step rollouts: twins with the same seeds with and without a normaliser."""
    import torch
    import rl_aerial_manipulator_amd as amd
    from rl_aerial_manipulator_amd.ppo import PPO
    from tests.test_gpu_ppo import fixture_policy, gae_magnitude
    n, T, gamma = 64, 96, 0.995

    def run(norm, bootstrap):
        env = amd.GpuWaypointEnv(n, seed=11, max_episode_steps=40)
        nz = amd.RewardNormalizer(n) if norm else None
        algo = PPO(env, policy=fixture_policy(env.device), n_steps=T, batch_size=n * T, n_epochs=1, seed=5, gamma=gamma, fused_rollout=fused,
                   bootstrap_truncated=bootstrap, reward_normalizer=nz)
        with torch.no_grad():
            algo.policy.log_std.data.fill_(-1.5)
        return algo, algo.collect_rollouts()

    (twin0, t0), (twin1, t1), (alg0, b0), (alg1, b1) = run(False, False), run(False, True), run(True, False), run(True, True)
    for b in (t1, b0, b1):
        assert torch.equal(b.actions, t0.actions) and torch.equal(b.dones, t0.dones)
    raw, dones = t0.rewards.cpu().numpy(), t0.dones.cpu().numpy()
    want = R.RetNormRef(n).block(raw, dones)
    check_outputs(b0.rewards.cpu().numpy(), want)
    # the twin's bootstrap gamma * V(terminal_obs): non-zero at its truncated entries only
    boot = (t1.rewards - t0.rewards).cpu().numpy()
    trunc = boot != 0
    assert 0 < trunc.sum() <= dones.sum() and (dones[trunc] != 0).all() and trunc[40].sum() > n // 2     # the 41st step is past the 40-step limit
    got0, got1 = b0.rewards.cpu().numpy(), b1.rewards.cpu().numpy()
    assert np.array_equal(got1[~trunc], got0[~trunc])
    # at the truncated entries the same bootstrap sits on top of the NORMALISED reward (added after the scaling, not scaled with it):
    # fp32 rounding of the three sums involved, plus the output tolerance of the normalised reward itself
    tol = 2e-6 + 2e-6 * np.abs(want) + 2.0 ** -22 * (np.abs(t1.rewards.cpu().numpy()) + np.abs(raw) + np.abs(got1))
    assert np.all(np.abs((got1 - want.astype(np.float32)) - boot)[trunc] <= tol[trunc])
    scale = np.abs(want / np.where(raw == 0, 1, raw))               # 1 / sigma_t (less where the reward was clipped)
    assert np.abs(boot * (1 - scale))[trunc].max() > 100 * tol[trunc].max()   # ... which a bootstrap scaled with the reward would miss by far
    # advantages are the GAE of the buffer's own rewards
    from oracle import oracle as O
    adv, _ = O.gae_reference(got1, b1.values.cpu().numpy(), dones, b1.last_values.cpu().numpy(), gamma, 0.9)
    mag = gae_magnitude(got1, b1.values.cpu().numpy(), dones, b1.last_values.cpu().numpy())
    assert (np.abs(b1.advantages.cpu().numpy() - adv) / (1.0 + mag)).max() < 1e-6   # the bound tests/test_gpu_ppo.py holds amenv_gae to
    # env.stats() stays raw: the episode returns of the twins agree
    assert alg1.env.stats()["return_sum"] == twin1.env.stats()["return_sum"]
    # checkpoints: one more member with a normaliser, the same members without; load continues with identical statistics
    p1, p0 = alg1.save(str(tmp_path / "with")), twin1.save(str(tmp_path / "without"))
    assert zipfile.ZipFile(p0).namelist() == ["policy.pth", "policy.optimizer.pth", "data"]
    assert zipfile.ZipFile(p1).namelist() == ["policy.pth", "policy.optimizer.pth", "data", "reward_normalizer.npz"]
    env = amd.GpuWaypointEnv(n, seed=11, max_episode_steps=40)
    fresh = PPO(env, policy=fixture_policy(env.device), n_steps=T, seed=5, fused_rollout=fused, reward_normalizer=amd.RewardNormalizer(n))
    fresh.load(p1)
    assert state_bytes(fresh.reward_normalizer) == state_bytes(alg1.reward_normalizer)
    r2, d2, _, _ = case(7, 64)
    assert (fresh.reward_normalizer.normalize(dev(r2), dev(d2)).cpu().numpy().tobytes()
            == alg1.reward_normalizer.normalize(dev(r2), dev(d2)).cpu().numpy().tobytes())
    twin1.load(p1)                                                # a model without a normaliser reads such a file too
    rec = alg1.train()
    assert all(np.isfinite(x) for x in rec.values())
