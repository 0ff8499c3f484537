"""The end of a lane-team step launch (hexacopter + arm, `step_kernel_team`): in the four + one geometry an integrating wave stores a
row's state, observation, reward, done and info bits BEFORE the kernel's barrier, and a row that ends its episode and resets rewrites them
behind it (same lane, same address: the later store wins); in both geometries terminal observation and Monitor's return / length are stored behind the barrier by the integrating
wave, the helper wave adds the ended episodes to the totals.  These tests pin that rewrite path where it can go wrong: every row of a
wave ending together, rows ending beside wave-mates that do not, partial row groups, one workgroup exactly, one workgroup plus a row, a
ragged last workgroup, the one + one geometry, fp32 and fp64 builds, auto-reset on and off.

Reference: the fp64 oracle, re-seated on the GPU state before every step (as tests/test_gpu_arm.py does), with that file's tolerances
(fp32: state 3e-6 relative, observation max(3e-6, 1.3e-7), flag flips <= 4 per run; fp64: 1e-12, no flips); reset STATES are bit-exact
against the oracle, fp32 reset OBSERVATIONS bit-exact against the one-lane-per-env kernel stepping the same state (same Philox words,
same fp32 arithmetic: the comparison test_team_kernel_tracks_the_lane_kernel makes; the fp64 builds round their rows to fp32 from
differently associated sums and are held to the oracle only)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_arm import both_step, orc_arm, rand_actions, reward_flips
from tests.test_gpu_parity import gpu_state, rel_err

pytestmark = pytest.mark.gpu

T = 4                                   # the task's time limit in these tests: every env ends on a known step (the one it takes with T steps behind it)
SIZES = [1, 3, 4, 16, 17, 20, 4100]     # partial row group | one wave | one workgroup | + one row | ragged last workgroup | one + one geometry
CASES = [(d, n) for d in ("f32", "f64") for n in SIZES]
TOL = {"f32": 3e-6, "f64": 1e-12}
STATE_ROWS = np.r_[0:15, 16:25]         # everything but the running episode return (the +2 bonus' threshold flips accumulate there)


def make(n, dtype, seed, auto_reset=True, kernel="team"):
    import rl_aerial_manipulator_amd as amd
    env = amd.GpuWaypointEnv(n, vehicle="hexa_arm", seed=seed, dtype=dtype, kernel=kernel, max_episode_steps=T, auto_reset=auto_reset)
    if kernel == "team":
        assert "step_kernel_team<" + ("float" if dtype == "f32" else "double") in env.kernel_name
        assert ("helper wave per 4" in env.kernel_name) == (n <= 4096), env.kernel_name     # four + one workgroups up to 4096 envs, one + one above
    env.reset()
    return env


def run_against_oracle(env, lane, orc, dtype, n, steps, actions, expect_done=None):
    """steps teacher-forced steps; returns (episode ends, sums of the per-step Monitor outputs) after checking every output of every step."""
    import torch
    tol = TOL[dtype]
    flips = bonus = 0
    tot = dict(episodes=0, truncated=0, terminated=0, crashed=0, length_sum=0, return_q10=0)
    for t in range(steps):
        a = actions(t)
        f0, i0 = env.get_state()
        lane.set_state(f0, i0)
        g, o = both_step(env, orc, a)
        ol = lane.step(torch.from_numpy(a).cuda())[0].cpu().numpy()
        f2, i2 = gpu_state(env)
        bad = (g["info"] & 127) != (o["info"] & 127)
        flips += int(bad.sum())
        ok = ~bad
        bonus += reward_flips(g, o, ok, dtype)
        done = o["done"] != 0
        assert np.array_equal(g["done"][ok], o["done"][ok])
        if expect_done is not None:
            assert np.array_equal(done, expect_done(t)), t
        # the reset bit: set on exactly the rows that ended (auto-reset is on in this run)
        assert np.array_equal((g["info"] & O.INFO_WAS_RESET) != 0, g["done"] != 0), t
        nd, dn = ok & ~done, ok & done
        assert np.array_equal(i2[:, ok], orc.istate[:, ok]), t
        if nd.any():
            assert rel_err(f2[STATE_ROWS][:, nd], orc.fstate[STATE_ROWS][:, nd]).max() < tol, t
        assert rel_err(g["obs"][ok], o["obs"][ok]).max() < max(tol, 1.3e-7), t
        if dn.any():
            assert np.array_equal(f2[:, dn], orc.fstate[:, dn]), t                       # reset state: bit-exact
            if dtype == "f32":
                assert np.array_equal(g["obs"][dn], ol[dn]), t                            # reset observation: bit-exact (fp32: the same arithmetic in both kernels)
            term = env.terminal_obs.cpu().numpy()
            assert rel_err(term[dn], o["terminal_obs"][dn]).max() < max(tol, 1.3e-7), t
            assert not np.array_equal(term[dn], g["obs"][dn]), t                          # ... and it is the row BEFORE the reset
            assert np.array_equal(env.ep_len.cpu().numpy()[dn], o["ep_len"][dn]), t
            er = env.ep_return.cpu().numpy().astype(np.float64)
            same_r = dn & (np.abs(g["reward"] - o["reward"]) < 1.0)                       # (not on the +2 bonus' threshold in this step: reward_flips counted those)
            assert (np.abs(er[same_r] - o["ep_return"][same_r]) <= (5e-5 if dtype == "f32" else 2e-7) * np.maximum(1.0, np.abs(o["ep_return"][same_r]))).all(), t
        gd = g["done"] != 0
        tot["episodes"] += int(gd.sum())
        term_bit = (g["info"] & O.INFO_TERMINATED) != 0              # (a row that crashes on the step of its time limit carries both bits and counts as terminated)
        tot["truncated"] += int((((g["info"] & O.INFO_TRUNCATED) != 0) & ~term_bit).sum()); tot["terminated"] += int(term_bit.sum())
        tot["crashed"] += int(((g["info"] & O.INFO_CRASHED) != 0).sum())
        tot["length_sum"] += int(env.ep_len.cpu().numpy()[gd].sum())
        tot["return_q10"] += int(np.rint(env.ep_return.cpu().numpy()[gd].astype(np.float32) * np.float32(1024.0)).astype(np.int64).sum())
    assert flips <= (4 if dtype == "f32" else 0), flips
    # The +2 progress bonus flips where rounding decides the sign of `last_distance - distance`.  These episodes are T + 1 steps long and
    # start at rest: the first steps move the vehicle by ~1e-5 m (0.4 g x (5 ms)^2 / 2 and its projection on the waypoint direction),
    # the distance of 1-3 m has an fp32 spacing of 1.2e-7..2.4e-7, so rounding decides a fraction of a percent of them -- the case
    # smoke() bounds at 1 % of the env-steps (tests/test_gpu_arm.py's 1e-4 is for 120-step episodes in motion).  fp64: none expected.
    assert bonus <= (0.01 if dtype == "f32" else 1e-4) * n * steps + 1, bonus
    return tot


def check_totals(env, tot, n, steps):
    st = env.stats()
    assert st["steps"] == n * steps
    for k in ("episodes", "truncated", "terminated", "crashed", "length_sum"):
        assert st[k] == tot[k], (k, st[k], tot[k])
    assert st["return_sum"] == tot["return_q10"] / 1024.0, (st["return_sum"], tot["return_q10"] / 1024.0)


@pytest.mark.parametrize("dtype,n", CASES)
def test_every_row_ends_on_the_time_limit(dtype, n):
    """max_steps = T from a staggered start (env i has i % T steps behind it): on every step a quarter of the rows ends -- rows next to
    wave-mates that go on; the second half of the batch (all of it below 8 envs) runs in step, so every row of its waves ends together."""
    rng = np.random.RandomState(n)
    env, lane = make(n, dtype, seed=21), make(n, dtype, seed=21, kernel="lane")
    orc = orc_arm(n, seed=21); orc.cfg.task.max_episode_steps = T
    f, i = gpu_state(env)
    phase = (np.arange(n) % T) * (np.arange(n) < 4 * (n // 8))          # the first half (whole row groups) staggered, the rest in step
    i[O.I_STEP] = phase
    env.set_state(f if dtype == "f64" else f.astype(np.float32), i)
    env.stats(reset=True)
    age = phase.copy()

    def expect(t):           # the time limit ends an episode on the step taken with T steps behind it: episodes of T + 1 steps
        d = age >= T
        age[:] += 1
        age[d] = 0
        return d
    steps = 3 * (T + 1)
    tot = run_against_oracle(env, lane, orc, dtype, n, steps, lambda t: rand_actions(rng, n), expect)
    assert tot["episodes"] == 3 * n and tot["truncated"] == tot["episodes"] and tot["length_sum"] >= 3 * n * (T + 1) - int(phase.sum())
    check_totals(env, tot, n, steps)
    env.close(); lane.close()


@pytest.mark.parametrize("dtype,n", CASES)
def test_some_rows_crash_beside_wave_mates_that_do_not(dtype, n):
    """Uniform actions from states near the crash height: some rows hit the ground on a step their wave-mates survive, the time limit
    ends the others."""
    rng = np.random.RandomState(100 + n)
    env, lane = make(n, dtype, seed=22), make(n, dtype, seed=22, kernel="lane")
    orc = orc_arm(n, seed=22); orc.cfg.task.max_episode_steps = T
    env.stats(reset=True)

    def lower(env):          # every third env just above the crash threshold and sinking, a few of the others tilted and spinning
        f, i = gpu_state(env)
        low = np.arange(n) % 3 == 0
        f[2, low] = rng.uniform(0.1005, 0.13, int(low.sum())); f[5, low] = rng.uniform(-2.0, -0.5, int(low.sum()))
        f[10:13, ::5] = rng.normal(0, 1.0, f[10:13, ::5].shape); f[22:25, ::7] = rng.normal(0, 1.0, f[22:25, ::7].shape)
        env.set_state(f if dtype == "f64" else f.astype(np.float32), i)
    crashed = episodes = 0
    steps = 0
    tot_all = None
    for rnd in range(3):     # 3 x (T + 1) steps, the states lowered again before each round
        lower(env)
        tot = run_against_oracle(env, lane, orc, dtype, n, T + 1, lambda t: rng.uniform(-1, 1, (n, 7)).astype(np.float32) * np.float32(0.5) + np.array([0.5, 0, 0, 0, 0, 0, 0], np.float32))
        tot_all = tot if tot_all is None else {k: tot_all[k] + v for k, v in tot.items()}
        steps += T + 1
    crashed, episodes = tot_all["crashed"], tot_all["episodes"]
    assert crashed >= 1 and (n < 3 or (crashed >= n // 6 and episodes > crashed)), (crashed, episodes)
    check_totals(env, tot_all, n, steps)
    env.close(); lane.close()


@pytest.mark.parametrize("dtype,n", CASES)
def test_without_auto_reset_an_ended_row_is_not_rewritten(dtype, n):
    """Auto-reset off: the step that ends an episode leaves the terminal state and the terminal observation in place (no reset bit, the
    same episode number), Monitor's outputs and totals still count the end."""
    rng = np.random.RandomState(200 + n)
    env = make(n, dtype, seed=23, auto_reset=False)
    orc = orc_arm(n, seed=23, flags=0); orc.cfg.task.max_episode_steps = T
    env.stats(reset=True)
    f, i = gpu_state(env)
    f[2, ::3] = 0.1005; f[5, ::3] = -1.0                                 # every third env crashes on the first step
    env.set_state(f if dtype == "f64" else f.astype(np.float32), i)
    ends = 0
    for t in range(T + 1):
        g, o = both_step(env, orc, rand_actions(rng, n))
        f2, i2 = gpu_state(env)
        assert np.array_equal(g["info"] & 127, o["info"] & 127) and np.array_equal(g["done"], o["done"]) and (g["info"] & O.INFO_WAS_RESET == 0).all()
        done = o["done"] != 0
        if t == 0:
            assert done[::3].all() and (n < 2 or not done.all())
        if t == T:
            assert done.all()                                             # the time limit, every row of every wave
        assert np.array_equal(i2, orc.istate) and (i2[O.I_EPISODE] == 1).all() and (i2[O.I_STEP] == t + 1).all()
        assert rel_err(f2[STATE_ROWS], orc.fstate[STATE_ROWS]).max() < TOL[dtype], t      # ended rows too: the state is the terminal one
        assert rel_err(g["obs"], o["obs"]).max() < max(TOL[dtype], 1.3e-7), t
        if done.any():
            assert np.array_equal(env.terminal_obs.cpu().numpy()[done], g["obs"][done]), t    # the observation row IS the terminal one
            assert np.array_equal(env.ep_len.cpu().numpy()[done], o["ep_len"][done])
        ends += int(done.sum())
    st = env.stats()
    assert st["episodes"] == ends and st["steps"] == n * (T + 1) and st["length_sum"] >= ends
    env.close()
