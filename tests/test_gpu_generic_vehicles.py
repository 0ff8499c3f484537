"""Every kernel family on the fully general vehicles of tests/generic_vehicles.py, against the fp64 oracle (`pytest -m gpu`).

The three default parameter sets are full of zeros and symmetries: diagonal inertias, one thrust range for all rotors, a symmetric rotor
layout, link 1's CoM at the joint, joint origins on an axis, symmetric joint limits (mid = 0), the reference's step length and episode
limits.  A kernel, or one of the places that pack amenv_vehicle for the device (make_hot, make_arm, make_quad, team_const_table,
make_team_params, the parameter blocks of the closed-loop and evaluation kernels, ee_home), that drops, transposes or mis-indexes a term
multiplied by one of those passes every test on them.  Here nothing is zero, equal or symmetric, and the step length, hold length and
time limit are others.  tests/test_generic_vehicles_cpu.py shows on the oracle alone that reverting any one group moves a step by 100
times the fp32 gate or more; tests/test_state_blob_cpu.py that the blobs reach every branch with no more envs near a threshold than the cap.

  (a) the branch sweep of tests/test_gpu_branch_sweep.py (its `_sweep`, `state_blob.compare` with its gates and flip rule unchanged)
  (b) reset, observe, forward kinematics, the tool point at home
  (c) amenv_arm_rhs: tests/test_gpu_arm.py::test_arm_right_hand_side_device_code_vs_oracle[*-generic]
  (d) amenv_rollout == steps, amenv_rollout_policy replays through steps, amenv_evaluate_policy == the twin's rollout reduced
  (e) randomisation, rotor lag and rate control (they scale, clamp with and multiply by the vehicle's own numbers) at their own tests' gates

  and the comparison can fail: a handle whose config carries one revert of the detection table is rejected in its first step.

Worst errors measured on the MI355X over the 24 sweep cases (6 steps x 300 envs each, 0 threshold flips), per family beside the default
vehicles' in DESIGN.md 4w:
  fp32: state 5.6e-6 (2-joint arm, team), reward 7.3e-6, observation rows 2.7e-7, ep_return 2.3e-6, terminal rows 1.7e-7
  fp64: state 1.1e-13, reward 1.7e-14, observation rows 1.2e-7 (one fp32 ulp: the team kernel's rows), ep_return 0, terminal rows 1.2e-7"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import generic_vehicles as GV
from tests import state_blob as B
from tests import test_gpu_branch_sweep as S
from tests.test_arm_cpu import rot_q
from tests.test_state_blob_cpu import oracle_cfg

pytestmark = pytest.mark.gpu

# (vehicle, task, kernel, dtype, substrings of kernel_name)
SWEEP = [
    ("gen_arm", "v2", "team", "f32", ("step_kernel_team<float",)), ("gen_arm", "v2", "team", "f64", ("step_kernel_team<double",)),
    ("gen_arm", "v2", "staged", "f32", ("step_kernel_armk<float",)), ("gen_arm", "v2", "staged", "f64", ("step_kernel_armk<double",)),
    ("gen_arm", "v2", "helper", "f32", ("step_kernel_arm2w",)),
    ("gen_arm", "v2", "lane", "f32", ("step_kernel<float", "arm3")), ("gen_arm", "v2", "lane", "f64", ("step_kernel<double", "arm3")),
    ("gen_arm_2j", "v2", "team", "f32", ("step_kernel_team<float", "2-joint arm")), ("gen_arm_base", "v2", "team", "f32", ("step_kernel_team<float",)),
    # axes other than (z, x, x): the general body, the lane kernel only
    ("gen_arm_yzx", "v2", "lane", "f32", ("step_kernel<float", "arm3")), ("gen_arm_yzx", "v2", "lane", "f64", ("step_kernel<double", "arm3")),
    ("gen_arm_skew", "v2", "lane", "f32", ("step_kernel<float", "arm3")), ("gen_arm_skew", "v2", "lane", "f64", ("step_kernel<double", "arm3")),
    ("gen_quad", "v2", "helper", "f32", ("step_kernel_pw<float,NROT=4",)), ("gen_quad", "v2", "lane", "f32", ("step_kernel<float,NROT=4",)),
    ("gen_quad", "v2", "lane", "f64", ("step_kernel<double,NROT=4",)), ("gen_quad", "v2", "team", "f32", ("step_kernel_quad<NROT=4",)),
    ("gen_hexa", "v2", "helper", "f32", ("step_kernel_pw<float,NROT=6",)), ("gen_hexa", "v2", "lane", "f32", ("step_kernel<float,NROT=6",)),
    ("gen_hexa", "v2", "lane", "f64", ("step_kernel<double,NROT=6",)), ("gen_hexa", "v2", "team", "f32", ("step_kernel_quad<NROT=6",)),
    # the other two compile-time task forms
    ("gen_quad", "v1_raw", "helper", "f32", ("step_kernel_pw<float,NROT=4,KW=2,v1>",)), ("gen_hexa", "v2k3", "lane", "f32", ("step_kernel<float,NROT=6,KW=4,v2>",)),
    ("gen_arm", "v2k3", "lane", "f32", ("step_kernel<float,NROT=6,KW=4,v2+arm3>",)),
]


@pytest.mark.parametrize("vehicle,task,kernel,dtype,names", SWEEP, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in SWEEP])
def test_every_branch_vs_oracle_on_generic_vehicles(vehicle, task, kernel, dtype, names):
    """Six teacher-forced steps of 300 envs (four whole 64-env tiles and a ragged one) from the generic blob: every output within
    `state_blob.compare`'s gates, the only excused envs those it excuses, every branch class reached, the Monitor totals."""
    S._sweep(f"test_every_branch_vs_oracle_on_generic_vehicles[{vehicle}-{task}-{kernel}-{dtype}]", vehicle, task, kernel, dtype, 300, names, None)


# the comparison can fail: a handle whose config carries ONE revert of the detection table against the oracle on the unreverted config
REVERTS = [("gen_quad", "lane", "Ixy <-> Ixz"), ("gen_hexa", "helper", "t_max of rotors 0, 1 swapped"), ("gen_hexa", "team", "mix row 3: rotors 0, 1 swapped"),
           ("gen_arm", "team", "link 1 inertia off-diagonals zeroed"), ("gen_arm", "team", "joint 2 mid zeroed"), ("gen_arm", "staged", "joint_origin[3] back to zero"),
           ("gen_arm", "helper", "link 1 CoM zeroed"), ("gen_arm_skew", "lane", "base inertia off-diagonals zeroed")]


@pytest.mark.parametrize("vehicle,kernel,label", REVERTS, ids=[f"{c[0]}-{c[1]}-{c[2]}".replace(" ", "_") for c in REVERTS])
def test_one_reverted_group_fails_the_comparison(vehicle, kernel, label):
    """What a kernel that ignored one parameter group would look like: `compare` rejects the first step (tests/test_generic_vehicles_cpu.py
    shows on the oracle that every revert of the table is this visible)."""
    import rl_aerial_manipulator_amd as amd
    n = 300
    cfg = S.generic_config(vehicle, n, kernel=kernel)
    dict(GV.mutations(cfg))[label](cfg)
    env = amd.GpuWaypointEnv(n, config=cfg)
    ocfg, _, _ = S.seat(env, vehicle, n)
    pre = S.gpu_state(env)
    a = B.actions(ocfg, pre[0], np.random.RandomState(S.ACTION_SEED))
    g = S.gpu_step(env, a)
    o, post = B.oracle_step(ocfg, pre, a)
    with pytest.raises(AssertionError):
        B.compare(g, o, B.margins(ocfg, pre, post), "f32")
    env.close()


# ---- (b) reset, observe, forward kinematics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicle,kernel", [("gen_arm", "lane"), ("gen_arm", "team"), ("gen_arm", "staged"), ("gen_arm_skew", "lane")])
def test_reset_observe_and_forward_kinematics_vs_oracle(vehicle, kernel):
    n = 300
    env = S.make_env(vehicle, n, kernel=kernel)
    cfg = oracle_cfg(vehicle, n)
    orc = O.OracleEnv(cfg)
    obs = env.reset().cpu().numpy().astype(np.float64)
    oobs = orc.reset()
    f, i = S.gpu_state(env)
    assert np.array_equal(f, orc.fstate) and np.array_equal(i, orc.istate), "reset state differs from the oracle"
    assert B.rel_err(obs, oobs).max() < B.REL32
    # random attitudes, joint angles and rates (the states of test_forward_kinematics_and_tool_point_task_vs_oracle)
    rng = np.random.RandomState(11)
    q = rng.normal(size=(4, n)); q[0] += 2; q /= np.linalg.norm(q, axis=0)
    f[6:10] = q
    f[19:22] = rng.uniform([[-3.1], [-1.5], [-1.5]], [[3.1], [1.5], [1.5]], (3, n))
    f[22:25] = rng.normal(0, 0.5, (3, n)); f[10:13] = rng.normal(0, 0.3, (3, n))
    env.set_state(f.astype(np.float32), i)
    f, i = S.gpu_state(env)
    orc.fstate[:] = f; orc.istate[:] = i
    assert np.abs(env.ee_position().cpu().numpy() - orc.ee_position()).max() < 2e-6
    assert B.rel_err(env.observe().cpu().numpy(), orc.observe()).max() < B.REL32
    # at home the tool point is the base position plus the sum of the three joint origins and the tool offset, turned by the attitude:
    # twelve numbers, none of them zero here
    v = cfg.vehicle
    home = np.array(v.joint_origin[:9]).reshape(3, 3).sum(0) + np.array(v.tool_offset[:3])
    assert (np.array(v.joint_origin[:9]) != 0).all() and (np.array(v.tool_offset[:3]) != 0).all()
    f[19:22] = 0.0
    env.set_state(f.astype(np.float32), i)
    f, i = S.gpu_state(env)
    want = np.stack([f[0:3, k] + rot_q(f[6:10, k]).T @ home for k in range(n)])
    assert np.abs(env.ee_position().cpu().numpy() - want).max() < 2e-6
    orc.fstate[:] = f
    assert B.rel_err(env.observe().cpu().numpy(), orc.observe()).max() < B.REL32
    env.close()


# ---- (d) the other launches carry the same parameters -------------------------------------------------------------------------------------------
ROLLOUT = [("gen_arm", "v2", "team", "step_kernel_team"), ("gen_arm", "v2", "lane", "step_kernel<float"), ("gen_quad", "v2", "team", "step_kernel_quad"),
           ("gen_hexa", "v2", "lane", "step_kernel<float,NROT=6"), ("gen_quad", "v1_raw", "helper", "step_kernel_pw<float,NROT=4,KW=2,v1>")]


@pytest.mark.parametrize("vehicle,task,kernel,name", ROLLOUT, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in ROLLOUT])
def test_rollout_from_the_generic_blob_equals_steps(vehicle, task, kernel, name):
    S.test_rollout_from_the_blob_equals_steps(vehicle, task, kernel, name)


POLICY = [("gen_arm", dict(kernel="team"), dict(kernel="team"), "step_kernel_team"), ("gen_arm", dict(kernel="lane"), dict(kernel="lane"), "step_kernel<float"),
          ("gen_quad", dict(), dict(kernel="team"), "step_kernel_quad<NROT=4"),
          ("gen_hexa", dict(kernel="lane", block_size=64), dict(kernel="lane", block_size=64), "step_kernel<float,NROT=6"),
          ("gen_quad", dict(kernel="helper", task="v1_raw"), dict(kernel="lane", task="v1_raw"), "step_kernel<float,NROT=4,KW=2,v1>")]


@pytest.mark.parametrize("vehicle,kw,twin_kw,twin_name", POLICY, ids=["gen_arm-team", "gen_arm-lane", "gen_quad-lane_quad", "gen_hexa-one_lane", "gen_quad-v1_raw-helper"])
def test_closed_loop_rollout_from_the_generic_blob_replays_through_steps(vehicle, kw, twin_kw, twin_name):
    S.test_closed_loop_rollout_from_the_blob_replays_through_steps(vehicle, kw, twin_kw, twin_name)


@pytest.mark.parametrize("vehicle,deterministic", [("gen_quad", True), ("gen_arm", False)])
def test_fused_evaluation_on_generic_vehicles_is_the_twin_rollout_reduced(vehicle, deterministic):
    """amenv_evaluate_policy packs the vehicle into a parameter block of its own: the comparison of tests/test_gpu_evaluate.py (counts equal,
    returns bit-equal to the host reduction of the one-lane-per-env rollout on a twin handle)."""
    from tests import test_gpu_evaluate as E
    n = 300
    env = S.make_env(vehicle, n, seed=12)
    twin = S.make_env(vehicle, n, seed=12, **(dict(kernel="lane") if vehicle == "gen_arm" else dict(block_size=64)))
    make = E.arm_policy(env.obs_dim, env.act_dim) if vehicle == "gen_arm" else E.fixture
    _, c, _, _ = E.check_against_twin(env, twin, make, per_env=1, max_steps=GV.MAX_EPISODE_STEPS + 2, deterministic=deterministic)
    assert c[:, 0].sum() == n
    env.close(); twin.close()


# ---- (e) the switches that read the vehicle ------------------------------------------------------------------------------------------------------
SWITCH_N, SWITCH_T = 200, 40          # (an episode of these vehicles runs into its time limit after 37 steps)


@pytest.mark.parametrize("vehicle", ["gen_quad", "gen_hexa"])
def test_randomisation_on_generic_vehicles_vs_the_per_env_oracle(vehicle):
    """The factors scale a FULL inertia and a mixer whose columns all differ: tests/dr_ref.py, the gate of
    tests/test_gpu_randomization.py::test_kernels_match_the_oracle_with_per_env_vehicles."""
    import rl_aerial_manipulator_amd as amd
    from tests import test_gpu_randomization as R
    wide = amd.DynamicsRandomization(mass=(0.6, 1.6), inertia=(0.5, 2.0), thrust=(0.8, 1.2))
    env = S.make_env(vehicle, SWITCH_N, seed=8, kernel="lane", randomization=wide)
    assert "+dr" in env.kernel_name
    R.check_against_per_env_oracle(env, "f32", SWITCH_T)
    env.close()


@pytest.mark.parametrize("vehicle", ["gen_quad", "gen_hexa"])
def test_rotor_lag_on_generic_vehicles_vs_the_pinned_oracle(vehicle):
    """Every rotor has thrust limits of its own: tests/lag_ref.py, the gate of tests/test_gpu_rotor_lag.py::test_lagged_kernels_match_the_pinned_oracle."""
    import rl_aerial_manipulator_amd as amd
    from tests import test_gpu_rotor_lag as LG
    lag = amd.RotorLag(0.015, 0.04)
    env = S.make_env(vehicle, SWITCH_N, seed=8, kernel="lane", rotor_lag=lag)
    LG.check_against_the_pinned_oracle(env, "f32", lag, None, SWITCH_T, vehicle)
    env.close()


@pytest.mark.parametrize("vehicle", ["gen_quad", "gen_hexa"])
def test_rate_control_on_generic_vehicles(vehicle):
    """The rate loop multiplies by the full nominal inertia: tests/rate_ref.py, the gates of
    tests/test_gpu_rate_control.py::test_moment_actions_are_the_restated_law and ::test_rate_mode_matches_the_oracle_fed_the_moment_rows."""
    import rl_aerial_manipulator_amd as amd
    from tests import test_gpu_rate_control as RC
    rate = amd.RateControl()
    law, env, twin = (S.make_env(vehicle, SWITCH_N, seed=8, kernel="lane", rate_control=rate) for _ in range(3))
    assert env.kernel_name.endswith(" +rate")
    RC.check_the_law(law, rate, vehicle)
    RC.check_against_the_oracle_fed_the_moment_rows(env, twin, vehicle, SWITCH_T)      # (env and twin: the same episodes from the same reset)
    law.close(); env.close(); twin.close()
