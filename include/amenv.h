/*
 * amenv.h -- C ABI of libamenv.so: the MI355X-resident batched waypoint environment.
 *
 * This is the drop-in boundary for ONE path of LahiruCooray/rl-aerial-manipulator:
 * `WaypointQuadEnv.step()/reset()` and the `simul_files` rigid-body integrator, stepped
 * for N independent environments per call instead of one.  The reference has no FFI
 * (it is pure Python); every entry point below names the reference interface it
 * replaces as  <file>:<line>  relative to the reference root, with
 *   v2 = initial-implementation-v2,  v1 = initial-implementation-v1.
 *
 * Conventions
 *  - plain C: pointers, sizes, fixed-width ints.  No torch / HIP types in signatures:
 *    a stream is passed as `void*` (a hipStream_t; NULL = the default stream).
 *  - all I/O buffers are DEVICE pointers owned by the caller (e.g. torch tensors);
 *    the library owns only its internal struct-of-arrays episode state.
 *  - every call only ENQUEUES work on the given stream: no hidden synchronisation, no
 *    allocation after amenv_create(), safe to capture into a hipGraph.
 *  - return value: 0 = AMENV_OK, negative = error code; text via amenv_last_error().
 *    Nothing throws, nothing calls exit().
 *  - one handle per device; calls on one handle are serialised by the caller.
 *    There is no global state: 8 handles on 8 GPUs can be driven from 8 processes/threads.
 */
#ifndef AMENV_H_
#define AMENV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMENV_ABI_VERSION 2

#define AMENV_MAX_ROTORS 8
#define AMENV_MAX_WAYPOINTS 4
#define AMENV_MAX_JOINTS 3
#define AMENV_MAX_ACTION_DELAY 8   /* control steps: 40 ms at 200 Hz (amenv_set_action_delay) */

/* error codes */
#define AMENV_OK 0
#define AMENV_ERR_INVALID -1   /* bad argument / config                       */
#define AMENV_ERR_HIP -2       /* a HIP runtime call failed (see last_error)   */
#define AMENV_ERR_NO_DEVICE -3 /* no usable gfx950 device                      */
#define AMENV_ERR_ALLOC -4

/* arithmetic type of the dynamics + episode state */
#define AMENV_F32 0 /* product path: fp32 SoA state, fp32 reward                         */
#define AMENV_F64 1 /* logic-check build of the SAME kernel in fp64 (reward/state fp64)  */

/* amenv_config.flags */
#define AMENV_FLAG_AUTO_RESET 1u /* SB3 VecEnv semantics: done envs are reset inside step()      */
/* AMENV_FLAG_NAN_GUARD (documented deviation): a step ends the episode with TERMINATED | NONFINITE (and TRUNCATED when the time limit was
 * reached), reward exactly -100, ep_return += -100, step += 1, when (a) any of the 13 + 2 n_joints state entries is non-finite after the
 * dynamics, or (b) any entry of the action row the step applies is non-finite (with an action delay: the delayed row that is applied, on
 * the step that applies it).  The terminal observation row of such an env is unspecified, and so is its float state when it is not reset.
 * Without the flag nothing is tested: a non-finite action entry is clamped to a rotor limit, which one is unspecified. */
#define AMENV_FLAG_NAN_GUARD 2u

/* amenv_config.step_kernel: which implementation of the SAME step amenv_step() launches.  All of them meet the parity
 * gate; LANE and HELPER are bit-identical to each other.  AUTO picks by batch size (latency regime vs throughput regime). */
#define AMENV_KERNEL_AUTO 0
#define AMENV_KERNEL_LANE 1   /* one lane per env, one wavefront per 64-env tile                                      */
#define AMENV_KERNEL_HELPER 2 /* LANE + helper wavefronts per tile (reset RNG words, observation rows, arm link 3)     */
#define AMENV_KERNEL_TEAM 3   /* arm vehicle: a team of 16 lanes (one DPP row) per env, AUTO up to 6144 envs; with AMENV_F64 the fp64 build of
                                 the SAME kernel (logic gate of its DPP plumbing; amenv_step only); rigid vehicles: 4 lanes (one DPP quad)
                                 per env, opt-in only (measured no faster than HELPER)                                       */
#define AMENV_KERNEL_STAGED 4 /* arm vehicle: the four RK4 stages' joint-configuration work on four wavefronts side by side,
                                 the base dynamics on their 36-number aggregates on a fifth (not bit-identical to LANE);
                                 AUTO for 6145..32768 envs; with AMENV_F64 the fp64 build of the same kernel (logic gate) */

/* amenv_task.ee_task (arm vehicles only; ignored without an arm) */
#define AMENV_EE_TASK_BASE 0 /* waypoint distance measured from the base position, as the reference's quadrotor task   */
#define AMENV_EE_TASK_TOOL 1 /* ... from the arm's tool point (forward kinematics): reward, reach test, obs[13:16]     */

/* task variants (which reference env file the step semantics follow) */
#define AMENV_TASK_V2_SCALED20 0 /* v2/rl_env_scaledObs.py  (20-D scaled obs) */
#define AMENV_TASK_V1_SCALED17 1 /* v1/rl_env_scaledObs.py  (17-D scaled obs) */
#define AMENV_TASK_V1_RAW17 2    /* v1/rl_env.py            (17-D raw obs)    */

/* info_bits[i], one uint32 per env per step (the reference's `info` dict + flags,
 * v2/rl_env_scaledObs.py:164,173,179,192,195,196) */
#define AMENV_INFO_TERMINATED 1u
#define AMENV_INFO_TRUNCATED 2u
#define AMENV_INFO_SUCCESS 4u
#define AMENV_INFO_STOPPED 8u
#define AMENV_INFO_CRASHED 16u
#define AMENV_INFO_OOB 32u
#define AMENV_INFO_NONFINITE 64u /* only with AMENV_FLAG_NAN_GUARD */
#define AMENV_INFO_WAS_RESET 128u /* this env was auto-reset at the end of this step */

/* Vehicle: n-rotor rigid body.  Replaces v2/simul_files/model/params.py:10-36.
 * All matrices row-major.  Rotor thrusts T = alloc . [F,Mx,My,Mz]^T, each clamped to
 * [t_min,t_max], then [F',Mx',My',Mz']^T = mix . T   (v2/simul_files/model/quadcopter.py:109-112). */
typedef struct amenv_vehicle {
  int32_t n_rotors; /* 1..AMENV_MAX_ROTORS */
  int32_t n_joints; /* 0 = rigid body; 1..3 = hexacopter + n-link arm (n < 3: the first n joints / links of the arrays below; same kernels,
                       the caller's dimensions: 4 + n actions, 20 + 2 n + 3 observations, 2 n joint state fields; amenv_step only) */
  double mass;      /* kg  (params.py:10) */
  double g;         /* m/s^2 (params.py:11) */
  double inertia[9];     /* body inertia I (params.py:12-14) */
  double inv_inertia[9]; /* I^-1 (params.py:16) */
  double alloc[AMENV_MAX_ROTORS * 4]; /* [n_rotors][4]  (params.py:36 invA) */
  double mix[4 * AMENV_MAX_ROTORS];   /* [4][n_rotors]  (params.py:31-34 A) */
  double t_min[AMENV_MAX_ROTORS];     /* per-rotor thrust floor (params.py:19, minF/4) */
  double t_max[AMENV_MAX_ROTORS];     /* per-rotor thrust cap   (params.py:20, maxF/4) */
  double moment_scale;   /* M = a[1:4]*moment_scale, evaluated in fp32 (rl_env_scaledObs.py:126: 0.1) */
  /* Arm (n_joints = 3): serial chain of revolute joints hanging from the base body; ignored for n_joints = 0.
   * With an arm, `mass` is the TOTAL mass (action scaling F = a0*mass*g), the base body's own mass is
   * mass - sum(link_mass), `inertia` is the base body's inertia about ITS CoM = the body-frame origin.
   * Parameters from Manipulator/src/manipulator_description/sdf/manipulator.sdf via tools/arm_params.py;
   * the joint servo model is this build's (no reference dynamics exist): DESIGN.md "arm". */
  double joint_origin[AMENV_MAX_JOINTS * 3]; /* joint k origin in its parent's frame (joint 1: body frame), :99,159,233 */
  double joint_axis[AMENV_MAX_JOINTS * 3];   /* unit axis (same in parent and child frame), :103,163,237 */
  double link_mass[AMENV_MAX_JOINTS];        /* :131,191,265 (+ closed gripper folded into link 3) */
  double link_com[AMENV_MAX_JOINTS * 3];     /* link CoM in its own frame */
  double link_inertia[AMENV_MAX_JOINTS * 9]; /* about the link CoM, link frame, row-major symmetric */
  double joint_kp, joint_kd;                 /* servo: thdd = clamp(kp*(cmd - th) - kd*thd, +-joint_acc_max) */
  double joint_acc_max;                      /* rad/s^2 (manipulator_moveit/config/joint_limits.yaml: 8) */
  double joint_reserved;
  double joint_limit[AMENV_MAX_JOINTS * 2];  /* [lower, upper] rad: action -1..1 maps onto it, :105-106,165-166,239-240 */
  double tool_offset[3];                     /* tool point in the last link's frame: midpoint of the two gripper-finger joint
                                                origins, manipulator.sdf:371,450 (forward kinematics -> amenv_ee_position, obs, task) */
} amenv_vehicle;

/* Task constants that the reference keeps as literals in rl_env_scaledObs.py. */
typedef struct amenv_task {
  int32_t variant;           /* AMENV_TASK_* */
  int32_t num_waypoints;     /* K; reference hard-codes 1 (rl_env_scaledObs.py:47); arm vehicles: 1 on every kernel, 2..4 on the LANE kernel */
  int32_t max_episode_steps; /* 2000 (rl_env_scaledObs.py:56) */
  int32_t counter_limit;     /* 500  (rl_env_scaledObs.py:59) */
  int32_t rk4_substeps;      /* RK4 sub-steps per control step; 1 */
  int32_t ee_task;           /* AMENV_EE_TASK_*: which point of an arm vehicle the waypoint task measures (default TOOL) */
  double dt;                 /* 1/200 (rl_env_scaledObs.py:30) */
  /* sin(2*pi*k/K), cos(2*pi*k/K), k = 1..K: used by the curved / helical waypoint
   * generators (v2/utils2/utils.py:39,46,53,83-87); filled by amenv_default_config(). */
  double traj_sin[AMENV_MAX_WAYPOINTS];
  double traj_cos[AMENV_MAX_WAYPOINTS];
} amenv_task;

typedef struct amenv_config {
  uint32_t struct_size; /* = sizeof(amenv_config): ABI guard */
  uint32_t abi_version; /* = AMENV_ABI_VERSION */
  int32_t num_envs;     /* N on THIS device */
  int32_t dtype;        /* AMENV_F32 | AMENV_F64 */
  uint32_t flags;       /* AMENV_FLAG_* */
  int32_t block_size;   /* 0 = auto; else threads per workgroup of the LANE kernel: 64, 128 or 256 */
  int32_t step_kernel;  /* AMENV_KERNEL_*: 0 = auto */
  int32_t reserved1;
  uint64_t seed;        /* reset RNG seed (Philox4x32-10 key) */
  int64_t env_id_offset; /* global id of local env 0: RNG is keyed by GLOBAL env id, so
                            results do not depend on how envs are sharded over GPUs */
  amenv_vehicle vehicle;
  amenv_task task;
} amenv_config;

/* Episode state, struct-of-arrays.  Float fields are `dtype` (fp32 or fp64), laid out
 * field-major: fstate[field][env], istate[field][env].  Replaces the attribute set of
 * WaypointQuadEnv (rl_env_scaledObs.py:26-38,53-77) + Quadcopter.state (quadcopter.py:28). */
enum amenv_float_field {
  AMENV_F_PX = 0, AMENV_F_PY, AMENV_F_PZ,          /* position            state[0:3]  */
  AMENV_F_VX, AMENV_F_VY, AMENV_F_VZ,              /* velocity            state[3:6]  */
  AMENV_F_QW, AMENV_F_QX, AMENV_F_QY, AMENV_F_QZ,  /* attitude quaternion state[6:10] */
  AMENV_F_WX, AMENV_F_WY, AMENV_F_WZ,              /* body rates p,q,r    state[10:13]*/
  AMENV_F_FINAL_YAW,                               /* rl_env_scaledObs.py:72          */
  AMENV_F_LAST_DISTANCE,                           /* :76 ; < 0 encodes None          */
  AMENV_F_EP_RETURN,                               /* Monitor-style running return    */
  AMENV_F_WP0                                      /* waypoints: WP0 + 3*k + {0,1,2}  */
  /* with n_joints = 3: joint angles (3) then joint rates (3) follow the waypoints: WP0 + 3*K + {0..5} */
};
enum amenv_int_field {
  AMENV_I_STEP = 0,   /* current_step (:55)                                         */
  AMENV_I_COUNTER,    /* counter (:57)                                              */
  AMENV_I_FLAGS,      /* bits 0-3 waypoint_index, bits 4-7 waypoints of this episode (v1 tasks; 0 = num_waypoints),
                         bit 8 final_waypoint_reached, bit 9 counter_activated */
  AMENV_I_EPISODE,    /* episodes started so far by this env (RNG counter)          */
  AMENV_I_NFIELDS
};
#define AMENV_FLAGBIT_FWR 256
#define AMENV_FLAGBIT_COUNTER_ACTIVE 512

/* Running totals since amenv_create / amenv_stats(reset=1): the Monitor / rollout
 * aggregates, reduced on the GPU (wavefront reduction + one atomic per wave). */
typedef struct amenv_stats {
  uint64_t steps;       /* env-steps executed */
  uint64_t episodes;    /* episodes finished  */
  uint64_t terminated, truncated, success, crashed, oob, nonfinite;
  uint64_t length_sum;  /* sum of finished episode lengths */
  int64_t return_sum_q10; /* sum of finished episode returns, fixed point 2^-10 (order-independent) */
} amenv_stats;

typedef struct amenv amenv; /* opaque */

/* ---- configuration helpers (host only, no device needed) ------------------------- */

/* Fill *cfg with the reference's own constants: the 0.18 kg quadrotor of
 * v2/simul_files/model/params.py and the v2 task literals.  vehicle_name:
 * "quad" (reference, oracle-pinned) | "hexa" | "hexa_arm" (hexacopter_description/
 * and Manipulator/ SDF parameters; no reference dynamics => parity unpinned). */
int amenv_default_config(const char* vehicle_name, int32_t num_envs, amenv_config* cfg);

/* Select which reference env file the task follows and fill that file's literals:
 * AMENV_TASK_V2_SCALED20 (v2/rl_env_scaledObs.py, 20-D obs, 2000 steps) or AMENV_TASK_V1_SCALED17 / _RAW17
 * (v1/rl_env_scaledObs.py / v1/rl_env.py: 17-D obs, 1..2 waypoints per episode, 1200 steps; used by v1/rl_train_vecN.py). */
int amenv_config_set_task(amenv_config* cfg, int32_t variant);

/* obs_dim / act_dim / number of float state fields for a config. */
int amenv_dims(const amenv_config* cfg, int32_t* obs_dim, int32_t* act_dim, int32_t* n_float_fields,
               int32_t* n_int_fields);

/* Algorithmic HBM bytes of one env-step of amenv_step() for this config (DESIGN.md formula). */
int64_t amenv_bytes_per_env_step(const amenv_config* cfg);

const char* amenv_version(void);

/* ---- lifetime --------------------------------------------------------------------- */

/* Replaces WaypointQuadEnv.__init__ (rl_env_scaledObs.py:10-38) x N and
 * make_vec_env(WaypointQuadEnv, n_envs=N) (v2/rl_train.py:24). */
int amenv_create(const amenv_config* cfg, int device, amenv** out);
int amenv_destroy(amenv* env);
/* Text of the last error on this handle (env may be NULL: last create error). */
const char* amenv_last_error(const amenv* env);

/* Re-key the reset RNG: episodes started after this call draw from (seed, global env id, episode).
 * Replaces the role of `np.random.seed(k)` in front of the reference env (its reset(seed=) is a no-op,
 * rl_env_scaledObs.py:41). */
int amenv_set_seed(amenv* env, uint64_t seed);

/* ---- the hot path ----------------------------------------------------------------- */

/* Replaces WaypointQuadEnv.reset (rl_env_scaledObs.py:40-79) for every env whose mask
 * byte is non-zero (mask NULL = all).  obs_out [N,obs_dim] f32 row-major may be NULL;
 * rows of un-reset envs are rewritten with their current observation. */
int amenv_reset(amenv* env, const uint8_t* mask, float* obs_out, void* stream);

/* Replaces, for all N envs in ONE kernel launch:
 *   WaypointQuadEnv.step          rl_env_scaledObs.py:123-196
 *   Quadcopter.update/state_dot   simul_files/model/quadcopter.py:66-114  (RK4 for odeint)
 *   _calculate_reward             rl_env_scaledObs.py:198-231
 *   _get_observation              rl_env_scaledObs.py:98-121
 *   quaternion_to_rpy             utils2/utils.py:4-9
 *   DummyVecEnv.step_wait auto-reset + Monitor episode stats (SB3; v2/rl_train.py:24)
 * actions      [N,act_dim] f32 row-major (already clipped by the caller, as SB3 does)
 * obs          [N,obs_dim] f32   next observation (post-reset for done envs when AUTO_RESET); obs_dim = 20 (v2 task),
 *              17 (v1 tasks), 29 with the arm: the 20 v2 entries + joint angles / pi (3) + joint rates / 5 (3) +
 *              (tool point - base position) / 0.5 in world axes (3)
 * reward       [N] f32 (f64 when dtype = AMENV_F64)
 * done         [N] u8   terminated|truncated
 * info_bits    [N] u32  AMENV_INFO_*
 * terminal_obs [N,obs_dim] f32 or NULL: row i written only when done[i]
 * ep_return    [N] f32 or NULL, ep_len [N] i32 or NULL: written only when done[i] */
int amenv_step(amenv* env, const float* actions, float* obs, void* reward, uint8_t* done,
               uint32_t* info_bits, float* terminal_obs, float* ep_return, int32_t* ep_len, void* stream);

/* amenv_step() plus the device-side duration of that one kernel: the launch carries start/stop
 * events stamped by the kernel's own dispatch (hipExtLaunchKernelGGL), then the call WAITS for the
 * stop event and writes the elapsed microseconds to *kernel_us (host pointer).  For bench/profiling
 * only: it synchronises. */
int amenv_step_timed(amenv* env, const float* actions, float* obs, void* reward, uint8_t* done,
                     uint32_t* info_bits, float* terminal_obs, float* ep_return, int32_t* ep_len, void* stream,
                     float* kernel_us);

/* T consecutive steps in ONE launch with open-loop actions [T,N,act_dim] (action replay /
 * action repeat).  Per-step outputs are [T,N,...] or NULL; state stays in registers between
 * steps.  Same per-step semantics as amenv_step (including auto-reset). */
int amenv_rollout(amenv* env, int32_t n_steps, const float* actions, float* obs, void* reward,
                  uint8_t* done, uint32_t* info_bits, void* stream);

/* ---- state access (parity injection, checkpoint/restore) --------------------------- */

/* Copy the whole SoA episode state to / from caller DEVICE buffers:
 * fstate [n_float_fields][N] of dtype, istate [AMENV_I_NFIELDS][N] int32. */
int amenv_get_state(amenv* env, void* fstate, int32_t* istate, void* stream);
int amenv_set_state(amenv* env, const void* fstate, const int32_t* istate, void* stream);

/* Recompute observations of the current state (no stepping): _get_observation, :98-121. */
int amenv_observe(amenv* env, float* obs_out, void* stream);

/* Forward kinematics of the arm (north_star "arm forward kinematics"): world position of the tool point of every env,
 * ee_out [N,3] f32.  Chain: base pose (p, q) -> joint origins / axes of manipulator.sdf:99,159,233 -> tool_offset (:371,450).
 * Without an arm (n_joints = 0) the tool point is the body origin.  The same quantity feeds obs[26:29] and, with
 * AMENV_EE_TASK_TOOL, the waypoint distance inside amenv_step. */
int amenv_ee_position(amenv* env, float* ee_out, void* stream);

/* Copy the running totals to *host_out (synchronises the stream); optionally zero them. */
int amenv_stats_read(amenv* env, amenv_stats* host_out, int reset, void* stream);

/* Bench / profiling only: copy `bytes` (a multiple of 16) with 4 or 16 bytes per lane -- a dispatch of known traffic in the access
 * pattern of the kernel under test, for calibrating the PMC counters FETCH_SIZE / WRITE_SIZE (tools/pmc_traffic.py). */
int amenv_calibration_copy(const void* src, void* dst, size_t bytes, int32_t bytes_per_lane, void* stream);

/* Name, VGPR count etc. of the step kernel chosen for this handle (for bench/profiles), formed from the handle's state at the time of
 * the call; the pointer is valid until the next call on the handle. */
const char* amenv_kernel_name(const amenv* env);

/* ---- observation normaliser: VecNormalize(norm_obs=True, norm_reward=False) (v1/rl_train_vecN.py:10-11) ------------
 * Running mean / variance / count of [n, dim] f32 observation batches on the device (SB3 2.6.0 RunningMeanStd:
 * initial mean 0, var 1, count 1e-4; parallel-moments merge), and obs_n = clip((obs-mean)/sqrt(var+eps), -clip, clip)
 * (SB3 defaults eps = 1e-8, clip = 10).  Third-party semantics, parity unpinned (the reference's vec_normalize.pkl is
 * a pickle and is not read). */
typedef struct amenv_obsnorm amenv_obsnorm;
int amenv_obsnorm_create(int32_t dim, int device, amenv_obsnorm** out);
int amenv_obsnorm_destroy(amenv_obsnorm* h);
/* obs_rms.update(obs): merge the moments of this batch (device pointer, row-major [n, dim]). */
int amenv_obsnorm_update(amenv_obsnorm* h, const float* obs, int64_t n, void* stream);
/* normalize_obs: out may alias in. */
int amenv_obsnorm_apply(amenv_obsnorm* h, const float* in, float* out, int64_t n, float clip, double eps, void* stream);
/* mean[dim], var[dim], count to / from HOST arrays (synchronises): save / load of the statistics. */
int amenv_obsnorm_get(amenv_obsnorm* h, double* mean, double* var, double* count, void* stream);
int amenv_obsnorm_set(amenv_obsnorm* h, const double* mean, const double* var, double count, void* stream);

/* ---- reward normaliser: the reward half of VecNormalize(norm_reward=True) -------------------------------------------
 * SB3's default, and the half amenv_obsnorm leaves out (the reference trains with norm_reward=False, v1/rl_train_vecN.py:11).
 * SB3 2.6.0 semantics restated, third-party, parity unpinned, checked against a numpy restatement.  A handle holds the discounted
 * return of every env, returns[N] (fp64, zero at creation and after reset_returns), and ONE scalar running mean / population variance /
 * count of those returns (initial 0 / 1 / 1e-4, as amenv_obsnorm).  Per env step t, training:
 *   1. returns = returns * gamma + r_t
 *   2. merge the batch (mean, population variance, N) of returns into the running statistics (the parallel-moments formula)
 *   3. out_t = clip(r_t / sqrt(var + eps), -clip, clip), var AFTER step 2
 *   4. returns[done_t] = 0
 * amenv_retnorm_rollout does this for the n_steps rows of a time-major block, in the order of t.  update != 0 is training; update == 0
 * is frozen: steps 1, 2 and 4 are skipped, every row is scaled with the variance at entry, the handle does not change (dones may then be
 * NULL).  Chunking guarantee: normalised rewards never feed back into a rollout, and the batch moments of a step depend on that step's
 * returns and N alone, so n_steps calls of one row, one call of n_steps rows and every other split of the same rows give bit-identical
 * outputs, statistics and returns; no floating-point atomics, so two runs from the same state are bit-identical too.  Blocks of any
 * length are accepted (the workspace, sized at creation, is reused every 128 rows).  fp64 returns and statistics.
 * SB3 defaults: gamma = .99, clip = 10, eps = 1e-8.  Refused with AMENV_ERR_INVALID before the device is queried or anything is
 * launched: num_envs <= 0, gamma outside [0, 1] or not finite, NULL out / handle / buffers, n_steps <= 0, clip <= 0, eps < 0;
 * AMENV_ERR_NO_DEVICE: no such HIP device. */
typedef struct amenv_retnorm amenv_retnorm;
int amenv_retnorm_create(int64_t num_envs, double gamma, int device, amenv_retnorm** out);
int amenv_retnorm_destroy(amenv_retnorm* h);
/* rewards_in / rewards_out [n_steps, N] f32 device buffers (may be the same), dones [n_steps, N] u8 (episode ended AT step t). */
int amenv_retnorm_rollout(amenv_retnorm* h, int32_t n_steps, const float* rewards_in, const uint8_t* dones, float* rewards_out, int32_t update,
                          float clip, double eps, void* stream);
/* VecNormalize.reset(): returns = 0; the statistics stay. */
int amenv_retnorm_reset_returns(amenv_retnorm* h, void* stream);
/* mean, var, count and (unless NULL) returns[N] to / from HOST memory (synchronises): save / load.  set with returns == NULL keeps them. */
int amenv_retnorm_get(amenv_retnorm* h, double* mean, double* var, double* count, double* returns, void* stream);
int amenv_retnorm_set(amenv_retnorm* h, double mean, double var, double count, const double* returns, void* stream);

/* ---- GPU-resident PPO helpers (SURVEY 8 row f3 / BASELINE config 5) ---------------------------------------------------
 * The reference trains with SB3 PPO (v2/rl_train.py:38-56).  The MLP stays in PyTorch-ROCm; these two entry points are
 * the per-env elementwise pieces of SB3's loop, on caller-owned device buffers of the CURRENT device.
 *
 * amenv_gae: RolloutBuffer.compute_returns_and_advantage (SB3 2.6.0) over time-major [n_steps, n_envs] f32 buffers;
 * dones[t, i] != 0 = env i's episode ended at step t (SB3's episode_starts shifted by one; the last row is its `dones`
 * argument); last_values[i] = V(obs after the last step).  gamma = .995, gae_lambda = .9 in the reference (:46-47). */
int amenv_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values, float* advantages,
              float* returns, int32_t n_steps, int64_t n_envs, float gamma, float gae_lambda, void* stream);
/* DiagGaussianDistribution.sample + log_prob + the action-space clip of collect_rollouts: raw = mean + exp(log_std) z,
 * clipped = clip(raw, low, high) (bounds v2/rl_env_scaledObs.py:20-24), logp = log N(raw; mean, exp(log_std)) summed over
 * act_dim (4; 5, 6 or 7 = 4 + the arm's joints).  z from Philox4x32-10 keyed by (seed, env_id_offset + i, draw): pass a different `draw`
 * per call.  Entry k draws block k / 4, entry k % 4 of it, whatever act_dim is: for the same key the first 4 + n entries of a 4 + n action
 * row are bit-identical to those of a 7-entry row with the same mean and log_std prefixes. */
int amenv_gaussian_act(const float* mean, const float* log_std, const float* low, const float* high, float* raw, float* clipped,
                       float* logp, int64_t n_envs, int32_t act_dim, uint64_t seed, uint32_t draw, int64_t env_id_offset, void* stream);
/* Forward pass of the reference's policy network (SB3 MlpPolicy, net_arch [128, 64, 64], tanh, separate actor / critic trunks;
 * v2/rl_train.py:27-30) in ONE launch: mean_out [n, act_dim] = action_net(pi trunk(obs)), value_out [n] = value_net(vf trunk(obs));
 * either output may be NULL.  flat_params = the policy's parameters in SB3 state-dict order in one contiguous fp32 buffer
 * (log_std, mlp_extractor.policy_net.{0,2,4}.{weight,bias}, mlp_extractor.value_net.{0,2,4}.{weight,bias}, action_net, value_net:
 * 30,537 floats for 20-D / 4-D).  (obs_dim, act_dim) in {(20,4), (29,7), (17,4), (25,5), (27,6), (24,4), (28,4), (21,4), (25,4)}: v2 |
 * hexacopter + 3-link arm | v1 | hexacopter + 1- / 2-link arm | the rigid vehicles' v2 rows with one / two action rows of history
 * (amenv_set_action_history) | their v1 rows with one / two.  Any other pair: AMENV_ERR_INVALID, nothing enqueued. */
int amenv_policy_forward(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, int64_t n, float* mean_out,
                         float* value_out, void* stream);

/* amenv_policy_forward for large batches (the rollout buffer's values / log-probabilities, a 32768-env policy step): the same outputs
 * from the training kernel's arithmetic -- fp32 products as six bf16 MFMAs on exactly split operands (see amenv_ppo_mlp_step) -- in two
 * launches (weight packing, forward); the (obs_dim, act_dim) pairs of amenv_policy_forward.  workspace: amenv_ppo_mlp_workspace_bytes() bytes, 16-byte aligned (the same area may serve
 * amenv_ppo_mlp_step: both rewrite its weight part from flat_params on every call). */
int amenv_policy_forward_mfma(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, int64_t n, float* mean_out,
                              float* value_out, void* workspace, void* stream);

/* Closed-loop rollout in ONE launch (SB3 collect_rollouts, v2/rl_train.py:38-56, for n_steps steps): per step
 *   obs_t -> actor / critic MLPs ([128, 64, 64] tanh; bf16 matrix cores, fp32 accumulate) -> a_t = mean + exp(log_std) z  (Philox keyed
 *   by (seed, global env id, draw0 + t) as amenv_gaussian_act) -> clip to the action box -> env step (as amenv_step, auto-reset included).
 * State, per-lane constants and the policy weights stay in registers between steps.  Built for fp32 vehicles:
 * the rigid vehicles with 4 or 6 rotors on every task -- on the single-waypoint v2 task with the default workgroup size the reference's
 * quadrotor (obs_dim 20, act_dim 4) runs the lane-quad step, 4 lanes per env: replaying the recorded clipped actions through amenv_step on
 * a handle created with AMENV_KERNEL_TEAM reproduces every row bit for bit; on the v1 tasks (obs_dim 17, v1/rl_train_vecN.py), the v2 task
 * with 2..4 waypoints or a set block_size one lane per env runs the arithmetic of the LANE / HELPER step kernels (replay through amenv_step
 * on a handle created with AMENV_KERNEL_LANE is bit for bit); both rigid forms run the first layer on two-part bf16 inputs and weights,
 * which holds the action within 3e-2 of the fp32 policy's on the reference checkpoint, and draw the same noise -- and the 6-rotor vehicle
 * with a 1-, 2- or 3-link arm (obs_dim 23 + 2 n, act_dim 4 + n) on the v2 task with 1..4 waypoints, any joint axes; fp64 envs return
 * AMENV_ERR_INVALID.  For the 3-link z,x,x arm on one waypoint the env part is the arithmetic of the kernel amenv_step runs for this env
 * (16 lanes per env where that is the lane-team kernel, else one lane per env with the arithmetic of the LANE / HELPER step kernels:
 * replaying the recorded clipped actions through amenv_step on such a handle reproduces every row bit for bit; a handle whose amenv_step
 * runs the STAGED kernel agrees to rounding); every other arm config runs the one-lane-per-env form at every batch size (replay through a
 * handle created with AMENV_KERNEL_LANE is bit for bit).  A 1- or 2-link arm publishes its own row widths (the columns amenv_step
 * returns); its phantom joints get 0 commands and no log-probability terms.  All forms draw the same noise.  An opt-in ROLLOUT mode: bf16
 * rounding perturbs the action means by ~1e-2 of their scale; log-probs are those of the samples under the means actually used.
 *   flat_params  fp32 policy parameters in SB3 state-dict order (see amenv_policy_forward)
 *   obs          [n_steps + 1, N, obs_dim] f32: row 0 <- observation at entry, row t + 1 <- after step t (post-reset for done envs)
 *   actions      [n_steps, N, act_dim] f32 raw (unclipped) samples;  logp, values, rewards [n_steps, N] f32;  dones [n_steps, N] u8
 *   info_bits    [n_steps, N] u32 or NULL;  terminal_obs [n_steps, N, obs_dim] f32 or NULL (rows written only where dones != 0) */
int amenv_rollout_policy(amenv* env, int32_t n_steps, const float* flat_params, uint64_t seed, uint32_t draw0, float* obs, float* actions,
                         float* logp, float* values, float* rewards, uint8_t* dones, uint32_t* info_bits, float* terminal_obs, void* stream);

/* amenv_rollout_policy with the observation normaliser INSIDE the launch: the rollout of `VecNormalize(env, norm_obs=True,
 * norm_reward=False)` (v1/rl_train_vecN.py:10-11) in one launch, for every fp32 rigid vehicle with 4 or 6 rotors (single-waypoint v2
 * included; always the one-lane-per-env form).  FROZEN-STATISTICS CONTRACT: the normaliser's mean / var are read once at entry and every
 * published observation -- obs rows 0..n_steps, the policy's input, terminal_obs rows -- is
 *   clip(float((double(raw) - mean) * (1 / sqrt(var + eps))), -clip, clip)
 * under those entry statistics, bit-identical to amenv_obsnorm_apply (SB3's VecNormalize updates them before every step instead).
 * update != 0: the raw rows 1..n_steps of every env (post-step / post-reset; not row 0, which the previous rollout or the caller's update
 * after reset counted; not the terminal rows, as SB3's VecNormalize) are summed in fp64 inside the launch and merged once afterwards
 * (amenv_obsnorm_update's merge with batch count n_steps x N: Chan's formula is associative, so the statistics equal n_steps per-step
 * updates to fp64 rounding).  update == 0 (VecNormalize.training = False) leaves the statistics untouched.  The normaliser's dim must be
 * the env's obs_dim and it must live on the env's device; arm vehicles, fp64 envs, NULL or bad arguments return AMENV_ERR_INVALID before
 * anything is launched.  clip, eps: VecNormalize's clip_obs (10) and epsilon (1e-8).  The other arguments are amenv_rollout_policy's. */
int amenv_rollout_policy_norm(amenv* env, amenv_obsnorm* norm, int32_t update, float clip, double eps, int32_t n_steps, const float* flat_params,
                              uint64_t seed, uint32_t draw0, float* obs, float* actions, float* logp, float* values, float* rewards, uint8_t* dones,
                              uint32_t* info_bits, float* terminal_obs, void* stream);

/* Closed-loop policy EVALUATION in ONE launch (SB3 evaluate_policy / EvalCallback): the loop of amenv_rollout_policy
 * -- obs -> MLPs (bf16 matrix cores) -> action -> clip -> env step with auto-reset -- with the episode accounting on the device and NO
 * per-step output.  Always the one-lane-per-env form (the arithmetic of amenv_rollout_policy[_norm] on a handle that runs that form,
 * applied action for applied action, bit for bit), 16 envs per workgroup (arm vehicles: 64) at every batch size.
 *   deterministic != 0: the applied action is clip(mean); == 0: the rollout's sample clip(mean + exp(log_std) z), z keyed by
 *                       (seed, global env id, draw0 + t) exactly as amenv_rollout_policy draws it
 *   norm               NULL, or the observation normaliser, FROZEN: its statistics are read at entry (amenv_rollout_policy_norm's
 *                       update == 0 semantics) and are bit-identical afterwards; clip, eps as there (ignored when norm is NULL)
 *   episodes_per_env   every env counts the first episodes_per_env episodes that END in it during the call; the episode already running
 *                       at entry counts when it ends.  An env that has filled its quota keeps stepping and adds nothing
 *   max_steps          the launch ends after max_steps steps, or as soon as every env has filled its quota (decided per workgroup)
 *   returns  [N][2] f64 device: sum and sum of squares of the counted episodes' returns (each the fp32 Monitor return, added in episode order)
 *   counts   [N][AMENV_EVAL_COUNT_COLS] i32 device: episodes, length_sum, success, crashed, out_of_bounds, truncated -- a flag column
 *            counts the episodes whose end bits carry AMENV_INFO_SUCCESS / _CRASHED / _OOB / _TRUNCATED (not exclusive of each other)
 *   steps_run [1] i32 device: the largest number of steps a workgroup executed; zeroed by the call, on the stream
 * No host sync, no allocation, graph-capturable.  AFTERWARDS the handle's state is wherever its lanes stopped (envs are mid-episode, and
 * not all at the same number of steps: amenv_reset before the handle is used for anything that needs a defined start); the Monitor totals
 * (amenv_stats) are UNTOUCHED: evaluation episodes and steps are not counted there.  Served: what amenv_rollout_policy[_norm] serve through
 * their one-lane-per-env kernels -- fp32 rigid vehicles with 4 or 6 rotors on every task with every admitted switch set, with or without
 * the normaliser; the 6-rotor vehicle with a 1..3-link arm on 1..4 waypoints (no normaliser).  AMENV_ERR_INVALID with a message naming
 * the reason, before anything is launched: NULL pointers; episodes_per_env <= 0 or max_steps <= 0; an fp64 handle; a handle without
 * AMENV_FLAG_AUTO_RESET; a rotor count other than 4 or 6; a normaliser on an arm vehicle, of the wrong dimension or on another device;
 * the normaliser together with the action history. */
#define AMENV_EVAL_COUNT_COLS 6   /* episodes, length_sum, success, crashed, out_of_bounds, truncated */
int amenv_evaluate_policy(amenv* env, amenv_obsnorm* norm /* NULL: none */, float clip, double eps, const float* flat_params, int32_t deterministic,
                          uint64_t seed, uint32_t draw0, int32_t episodes_per_env, int32_t max_steps, double* returns /* [N][2]: sum, sum of squares */,
                          int32_t* counts /* [N][6] */, int32_t* steps_run /* [1], device */, void* stream);

/* ---- per-episode dynamics randomisation --------------------------------------------------------------------
 * For every env and every episode the rigid vehicle's mass, inertia and rotor thrusts are scaled by factors drawn uniformly:
 *   km  mass factor: the body's mass is km * m.  Action scaling keeps the NOMINAL mass (F = a0 * m * g in fp32, as without), so the
 *       policy's "1.0 = hover" is off by km, as on a real vehicle carrying a different payload;
 *   kI  inertia factor: the body's inertia is kI * I;
 *   s_r thrust factor of rotor r, one draw per rotor: the rotor delivers s_r * clamp(t_r, t_min_r, t_max_r) (commands still saturate at
 *       the nominal limits).
 * Dynamics: F = sum_r s_r t_r, M = mix[1..3] (s . t); translational acceleration F / (km m); rotational J (M / kI - w x I w), which is
 * (kI I)^-1 (M - w x (kI I) w).  Gravity, task, reward, observation, reset draws and the Monitor totals are unchanged; the factors are
 * not observed.
 * Draw: ONE Philox4x32-10 block, key = the config seed (amenv_set_seed re-keys it), counter = (global env id lo, hi, episode,
 * 0x44520000), cut into eight 16-bit uniforms u[2k] = (w[k] & 0xffff) * 2^-16, u[2k+1] = (w[k] >> 16) * 2^-16; u[0] -> km, u[1] -> kI,
 * u[2 + r] -> s_r; factor = lo + (hi - lo) * u in fp32 (a multiply, then an add).  The factors are a pure function of (seed, global env
 * id, episode, ranges): no state is stored (state layout, get / set_state and sharding are unaffected), and a change of ranges applies
 * from the next launch ON, to episodes already running too (curricula rely on this).
 * Served: rigid vehicles with 4 or 6 rotors, fp32 and fp64, by amenv_step / amenv_step_timed / amenv_rollout (lane and helper-wave
 * kernels) and amenv_rollout_policy / amenv_rollout_policy_norm (one lane per env: a config the lane-quad closed loop would serve runs
 * the one-lane-per-env form instead while randomisation is on).  Refused with AMENV_ERR_INVALID, before anything is launched: arm
 * vehicles, other rotor counts, a handle whose step kernel is the lane-quad one (step_kernel = AMENV_KERNEL_TEAM on a rigid vehicle), a
 * bad struct_size, ranges that are not finite with 0.25 <= lo <= hi <= 4. */
typedef struct amenv_randomization {
  uint32_t struct_size;  /* = sizeof(amenv_randomization): guard */
  uint32_t reserved;
  float mass_scale[2];   /* [lo, hi]; {1, 1} = fixed */
  float inertia_scale[2];
  float thrust_scale[2]; /* drawn independently per rotor */
} amenv_randomization;
/* r NULL = off (the nominal vehicle). */
int amenv_set_randomization(amenv* env, const amenv_randomization* r);
/* out [N, 2 + n_rotors] f32 (device): km, kI, s_0 .. s_{n_rotors-1} of every env's current episode; all 1 when off. */
int amenv_dynamics_factors(amenv* env, float* out, void* stream);

/* ---- first-order rotor lag ---------------------------------------------------------------------------------
 * Opt-in, per handle.  Per env and rotor there is one more state number w_r >= 0, the square root of the thrust the rotor delivers
 * (thrust = k_f speed^2: w_r is the rotor speed up to the constant sqrt(k_f)).  Once per control step, in place of "use the clamped thrust":
 *   t_c  = clamp(alloc[r] . u, t_min[r], t_max[r])      exactly as without the lag
 *   c    = sqrt(t_c);   a = c > w_r ? a_up : a_down;   w_r' = fma(a, c - w_r, w_r);   the rotor delivers t_r = w_r' * w_r'
 * then t_r *= s_r if randomisation is on, and the mix / RK4 as without.  t_r is held over the whole control step (every RK4 stage and
 * sub-step); w_r' is the new state.  a_up = -expm1(-dt / tau_up), a_down = -expm1(-dt / tau_down), formed in fp64 from task.dt (the
 * control period) and rounded once to the handle's dtype.  fp32 handles take the square root with v_sqrt_f32 (1 ulp).
 * Episode start: w0_r = sqrt(clamp(alloc[r] . (mass g, 0, 0, 0), t_min[r], t_max[r])) with the NOMINAL mass, fp64 rounded once: the rotors
 * spin at the nominal hover command.  An env gets w <- w0 when its episode starts (auto-reset inside a step or rollout, amenv_reset for the
 * masked envs); with auto-reset off an env that ended keeps its rotor state like the rest of its state.  Turning the lag on where it was
 * off sets every env's rotor state to w0; new time constants on a handle where it is on keep the states and apply from the next launch.
 * The rotor state is not observed and is no part of amenv_get_state / amenv_set_state, whose layout does not change; it draws nothing, so
 * sharding by global env id is unaffected.  Reward, task, reset draws and Monitor totals are unchanged.
 * Served: what amenv_set_randomization serves, and composable with it (rigid vehicles with 4 or 6 rotors, fp32 and fp64, lane and
 * helper-wave step kernels, amenv_rollout, amenv_rollout_policy[_norm] in the one-lane-per-env form).  Refused with AMENV_ERR_INVALID before
 * anything is launched or changed: arm vehicles, other rotor counts, a handle whose step kernel is the lane-quad one, any t_min[r] < 0, a
 * bad struct_size, a time constant that is not finite with 0 < tau <= 10.
 * amenv_set_rotor_lag is a configuration call: it is the only one of the three that may allocate (the side buffer of rotor states, on the
 * first enable) and it may synchronise the device; do not call it inside a stream capture.  amenv_get / set_rotor_state only enqueue, as
 * step, rollout and reset do with the lag on. */
typedef struct amenv_rotor_lag {
  uint32_t struct_size;   /* = sizeof(amenv_rotor_lag): guard */
  uint32_t reserved;
  double tau_up, tau_down;  /* seconds; model.sdf timeConstantUp / timeConstantDown: 0.015 */
} amenv_rotor_lag;
/* lag NULL = off: the handle launches exactly the kernels it launched before. */
int amenv_set_rotor_lag(amenv* env, const amenv_rotor_lag* lag);
/* [N, n_rotors] of the handle's dtype, row-major (device): w_r of every env.  Refused while the lag is off. */
int amenv_get_rotor_state(amenv* env, void* out, void* stream);
/* the inverse: parity injection, checkpoint / restore.  Refused while the lag is off. */
int amenv_set_rotor_state(amenv* env, const void* in, void* stream);

/* ---- sensor noise on the observations ----------------------------------------------------------------------
 * Opt-in, per handle, all standard deviations 0 by default.  Every observation row a kernel forms -- the step row, the terminal row, the
 * post-reset row, the amenv_reset row, the amenv_observe row, every row of amenv_rollout and amenv_rollout_policy[_norm] -- is formed from a
 * perturbed COPY of the 13 state numbers; the state itself, reward, termination, the reset draws, amenv_get_state, amenv_ee_position and
 * the Monitor totals use the true state.  The noise is a pure function of (config seed, global env id, episode, s), s = the env's step
 * field as stored after the row's step (0 for a post-reset row): no state is stored, sharding by global env id is unaffected, a run can be
 * replayed, and amenv_observe returns the row the last step returned.
 *   draw    three Philox4x32-10 blocks, key = seed, counter = (gid lo, gid hi, episode, 0x4E000000 | ((s & 0x3FFFFF) << 2) | b), b = 0, 1, 2;
 *           word k of block b is sample j = 4 b + k:  n_j = (float(sum of the word's four bytes) - 510.0f) * 0.006765875f
 *           (unit variance, |n| <= 3.4506, excess kurtosis -0.3: an Irwin-Hall sum of four byte-uniforms; no Box-Muller, so the samples
 *           are integer arithmetic and one multiply, reproducible bit for bit on a CPU)
 *   j 0..2  p += sigma_position n     j 3..5  v += sigma_velocity n     j 6..8  w += sigma_rate n          (one fma each)
 *   j 9..11 d = (sigma_attitude / 2) n;  q~ = q (x) (1, d) (Hamilton product, scalar first), renormalised
 * With the observation normaliser inside amenv_rollout_policy_norm the noise comes first: the frozen statistics normalise the noisy row
 * and the `update` sums count the noisy raw rows.
 * Served: fp32 handles of what amenv_set_randomization serves (rigid vehicles with 4 or 6 rotors, every task, lane and helper-wave step
 * kernels, amenv_rollout, amenv_rollout_policy[_norm] in the one-lane-per-env form), composable with randomisation and rotor lag.
 * Refused with AMENV_ERR_INVALID, the handle untouched: a bad struct_size, a sigma that is not finite with 0 <= sigma <= 1, arm vehicles,
 * other rotor counts, fp64 handles, a handle whose step kernel is the lane-quad one, task.max_episode_steps > 2^22 - 2 (s has 22 bits).
 * A configuration call without allocation or launch; it applies from the next launch. */
typedef struct amenv_sensor_noise {
  uint32_t struct_size;   /* = sizeof(amenv_sensor_noise): guard */
  float sigma_position;   /* m */
  float sigma_velocity;   /* m/s */
  float sigma_rate;       /* rad/s */
  float sigma_attitude;   /* rad */
} amenv_sensor_noise;
/* z NULL or all sigmas 0 = off: the handle launches exactly the kernels it launched before. */
int amenv_set_sensor_noise(amenv* env, const amenv_sensor_noise* z);
/* out [N, 12] f32 (device): the twelve unit samples n_0 .. n_11 of every env's current (episode, step), whether the noise is on or off. */
int amenv_sensor_noise_samples(amenv* env, float* out, void* stream);

/* ---- per-episode actuation latency ---------------------------------------------------------------------------
 * Opt-in, per handle, off by default.  Each env has an integer delay d, drawn when its episode starts and fixed for that episode, and a
 * history of the last 8 action rows it was GIVEN (4 floats each, the caller's row as passed; in amenv_rollout_policy[_norm] the clipped
 * sample).  A step with given row a applies a if d = 0, else the row given d steps ago, to the dynamics (fp32 action scaling, mixer, clamp,
 * lag filter, thrust factors: all unchanged and in the same order); then a enters the history.  Where the episode is younger than d steps
 * the applied row is the hover row (1, 0, 0, 0).  Nothing else changes: reward, task, observation (neither d nor the pending rows are
 * observed), reset draws, Monitor totals, amenv_dims, the state layout, amenv_get_state / amenv_set_state; `actions` and `logp` of the
 * closed loop record the policy's own samples.
 *   draw    one Philox4x32-10 block, key = seed, counter = (gid lo, gid hi, episode, 0x4C540000), episode = AMENV_I_EPISODE while that
 *           episode runs;  d = min_steps + (((w0 >> 16) * (max_steps - min_steps + 1)) >> 16)   (integer arithmetic only)
 *   start   an auto-reset inside a step or rollout, and amenv_reset for the masked envs: d is drawn for the new episode number and all 8
 *           history rows become hover.  With auto-reset off a finished env keeps both.
 *   on/off  off -> on: every env draws d for its current episode and gets hover rows.  A new range on a handle where it is on keeps every
 *           env's d and history and applies to the episodes that start afterwards.  amenv_set_state does not touch d or the history
 *           (their order does not depend on the step field); amenv_set_seed re-keys the draws of later episodes only.
 * Served: fp32 handles of what amenv_set_randomization serves (rigid vehicles with 4 or 6 rotors, every task, lane and helper-wave step
 * kernels, amenv_rollout, amenv_rollout_policy[_norm] in the one-lane-per-env form), composable with randomisation, rotor lag and sensor
 * noise in every combination.
 * Refused with AMENV_ERR_INVALID, the handle untouched: a bad struct_size, min_steps < 0, min_steps > max_steps, max_steps >
 * AMENV_MAX_ACTION_DELAY, arm vehicles, other rotor counts, fp64 handles, a handle whose step kernel is the lane-quad one.
 * A configuration call like amenv_set_rotor_lag: the first enable allocates the side buffer (132 B per env) and off -> on synchronises;
 * not to be called inside a stream capture. */
typedef struct amenv_action_delay {
  uint32_t struct_size;            /* = sizeof(amenv_action_delay): guard */
  int32_t min_steps, max_steps;    /* control steps, 0 <= min_steps <= max_steps <= AMENV_MAX_ACTION_DELAY */
} amenv_action_delay;
/* z NULL = off: the handle launches exactly the kernels it launched before. */
int amenv_set_action_delay(amenv* env, const amenv_action_delay* z);
/* d_out [N] int32, recent_out [N, 8, 4] f32 in AGE order (row k was given k + 1 steps ago; hover where the episode is younger), device
 * pointers, recent_out 16-byte aligned; either may be NULL.  Only enqueues.  Refused while the delay is off. */
int amenv_get_action_delay_state(amenv* env, int32_t* d_out, float* recent_out, void* stream);
/* the inverse: checkpoint / restore, parity injection; either may be NULL (that part stays).  d is clamped to 0..8 by the kernel (the
 * pointers are device memory: the host cannot check them).  Only enqueues.  Refused while the delay is off. */
int amenv_set_action_delay_state(amenv* env, const int32_t* d_in, const float* recent_in, void* stream);

/* ---- action history in the observation rows -------------------------------------------------------------------
 * Opt-in, per handle, off by default; composes with randomisation, rotor lag, sensor noise and the action delay in every combination.
 * While it is on with H = rows (1 or 2), every observation row the library publishes is the task's row followed by the last H action rows
 * the env was GIVEN, most recent first: obs_dim = base + 4 H, base = 20 (v2 task) or 17 (v1 tasks).  Columns base + 4 k .. base + 4 k + 3
 * hold the row given k + 1 steps ago in this episode, bit for bit as the caller passed it (in amenv_rollout_policy the clipped sample, as
 * for the delay): raw values, thrust / (m g) in [0, 2] and moments in [-1, 1], not scaled, not perturbed by the sensor noise, not replaced
 * by the applied row.  Where the episode is younger than k + 1 steps the columns hold the hover row (1, 0, 0, 0).  They are the first H rows
 * of what amenv_get_action_delay_state publishes as recent_out, after the step's push.
 *   step row of an env that goes on                   [a_t, a_{t-1}]
 *   terminal row (written where done)                 [a_t, a_{t-1}]: the history before the reset wipes it
 *   post-reset row of an auto-reset env,
 *   amenv_reset row of a masked env                   hover rows
 *   amenv_reset row of an unmasked env, amenv_observe the env's current history
 *   rows of amenv_rollout / amenv_rollout_policy      as the same steps through amenv_step publish them (row 0 of the closed loop: the
 *                                                     current history)
 * The history IS the delay's side buffer.  With the delay off the delay machinery runs with range (0, 0): every d is 0, the applied row is
 * the given row and the dynamics are bit-identical to a handle without either.  Turning the history on where neither was on allocates the
 * buffer (a configuration call like amenv_set_action_delay: it may allocate and synchronise, not inside a stream capture) and fills it with
 * hover rows; where the delay is on, the history shows the rows the delay has kept.  amenv_set_action_delay keeps its rules (off -> on draws
 * d and fills hover rows, a new range keeps d and the rows); while the history is on, amenv_set_action_delay(NULL) means range (0, 0) for
 * the episodes that start afterwards and the buffer stays.  amenv_get/set_action_delay_state work while either is on.
 * Nothing else changes: reward, task, state layout, amenv_get_state / amenv_set_state, reset draws (nothing is drawn: sharding by global env
 * id holds), Monitor totals, amenv_dims(cfg), amenv_bytes_per_env_step(cfg).
 * Served: fp32 handles of what amenv_set_action_delay serves, through amenv_step, amenv_step_timed, amenv_rollout, amenv_reset,
 * amenv_observe and amenv_rollout_policy in the one-lane-per-env form (a config the lane-quad closed loop would serve runs the one-lane form
 * while the history is on).  Every obs / terminal_obs buffer passed while it is on has rows of amenv_obs_dim(env) floats.
 * Refused with AMENV_ERR_INVALID, the handle untouched: rows outside 0..2, arm vehicles, other rotor counts, fp64 handles, a handle whose
 * step kernel is the lane-quad one; and amenv_rollout_policy_norm while the history is on (normalise step by step).
 * amenv_policy_forward, amenv_policy_forward_mfma and amenv_ppo_mlp_step accept the (obs_dim, act_dim) pairs (24, 4), (28, 4), (21, 4), (25, 4). */
/* rows = 0: off (the handle publishes base-width rows and, if the delay is off too, launches exactly the kernels it launched before) */
int amenv_set_action_history(amenv* env, int32_t rows);
/* the row width every obs / terminal_obs buffer of this handle must have now: base + 4 rows */
int32_t amenv_obs_dim(const amenv* env);

/* ---- body-rate actions with an inner rate loop -----------------------------------------------------------------
 * Opt-in, per handle, off by default; composes with randomisation, rotor lag, sensor noise, the action delay and the action history.
 * While it is on, entries 1..3 of an action row are body-rate COMMANDS in units of max_rate (the thrust entry keeps its meaning), and a
 * rate loop inside the step turns them into the moment action the unchanged step consumes.  With a the row the step is about to apply
 * (behind the latency: the delayed command), w the env's body rates at the start of the step, I the NOMINAL inertia of the config (not the
 * randomised one) and ms = task.moment_scale, in fp32 and in this order:
 *   w_cmd_k = a_k * max_rate_k;   u_k = gain_k * (w_cmd_k - w_k);   tau = I u  (+ w x (I w) with gyro_feedforward);   a'_k = tau_k * float(1 / ms)
 * Everything behind a' is the step as without the switch: M = a' * ms, mixer, per-rotor clamp, lag, RK4, reward, observation.  Nothing clips
 * a'; the rotor clamp is the actuator limit.  The loop is proportional plus feed-forward and keeps no state: the state layout, amenv_get_state
 * / amenv_set_state, the reset draws and sharding by global env id are unaffected.  The rows of the action history, of the delay's buffer and
 * of the closed loop's `actions` are the commands as given, never a'.
 * Served: fp32 handles of what amenv_set_action_delay serves (rigid vehicles with 4 or 6 rotors, every task, lane and helper-wave step
 * kernels, amenv_rollout, amenv_rollout_policy[_norm] and amenv_evaluate_policy in the one-lane-per-env form: a config the lane-quad closed
 * loop would serve runs the one-lane form while rate control is on).
 * Refused with AMENV_ERR_INVALID, the handle untouched: arm vehicles, other rotor counts, fp64 handles, a handle whose step kernel is the
 * lane-quad one, a max_rate or gain that is not finite and > 0, gain_k * task.dt >= 1 (past that bound the held torque overshoots the
 * command within one step).  A configuration call without allocation or launch; it applies from the next launch. */
typedef struct amenv_rate_control {
  double max_rate[3];        /* rad/s per unit of action, body x, y, z */
  double gain[3];            /* 1/s */
  int32_t gyro_feedforward;  /* != 0: add w x (I w) */
  int32_t reserved;
} amenv_rate_control;
/* r NULL = off: the handle launches exactly the kernels it launched before. */
int amenv_set_rate_control(amenv* env, const amenv_rate_control* r);
/* actions [N, 4] f32 commands, out [N, 4] f32 (device; may be the same buffer): [a_0, a'_x, a'_y, a'_z] from the handle's CURRENT body rates
 * by the kernels' own device function.  It converts the rows it is given: the latency is ignored.  Only enqueues.  Refused while rate
 * control is off. */
int amenv_rate_moment_actions(amenv* env, const float* actions, float* out, void* stream);

/* ---- per-episode rotor failure -----------------------------------------------------------------------------------
 * Opt-in, per handle, off by default; composes with randomisation, rotor lag, sensor noise, the action delay, the action history and
 * rate control.  With `probability` an episode has ONE failure: one rotor, drawn among those of rotor_mask, delivers from control step
 * `onset` of the episode on only the fraction f (`remaining`, 0 = a dead rotor) of what it would deliver.  The plan is a pure function of
 * (seed, global env id, episode, these parameters), with no stored state: ONE Philox4x32-10 block, key = the config seed, counter
 * (gid lo, gid hi, episode, 0x46410000), cut into 16-bit halves v0..v3 (low / high half of word 0, low / high half of word 1):
 *   failure iff v0 < floor(probability * 65536 + 0.5)       (an integer compare: 0 never fails, 1 always)
 *   rotor  = the k-th set bit of rotor_mask in ascending order, k = (v1 * popcount(rotor_mask)) >> 16
 *   onset  = onset_min + ((v2 * (onset_max - onset_min + 1)) >> 16)
 *   f      = remaining_min + (remaining_max - remaining_min) * (float(v3) * 2^-16)      (fp32: a multiply, then an add)
 * In every control step whose step field, as the step finds it (istate[AMENV_I_STEP]), is >= onset, the failed rotor's thrust factor is
 * s'_r = s_r * f (one rounded multiply in the handle's dtype), wherever the step uses s_r (amenv_set_randomization): F = sum s_r t_r,
 * M = mixm (s . t), with the rotor lag on the delivered w'^2.  Commands still clamp at the nominal limits and the lag state keeps
 * following the command.  Action scaling, reward, observation, reset draws, Monitor totals and the state layout are untouched; the failure
 * is not observed.  The compare is on the loaded step, so amenv_set_state into the middle of an episode behaves as running up to that
 * step; new parameters apply from the next launch, to running episodes too.
 * Served: what amenv_set_randomization serves (rigid vehicles with 4 or 6 rotors, fp32 and fp64, lane and helper-wave step kernels,
 * amenv_rollout, amenv_rollout_policy[_norm] and amenv_evaluate_policy in the one-lane-per-env form).  Refused with AMENV_ERR_INVALID, the
 * handle untouched: arm vehicles, other rotor counts, a handle whose step kernel is the lane-quad one, a wrong struct_size, a probability
 * that is not finite in 0..1, an onset range outside 0 <= min <= max <= 65535, a remaining range that is not finite with
 * 0 <= min <= max <= 1, a rotor_mask bit at or above n_rotors.  A configuration call without allocation or launch. */
typedef struct amenv_rotor_failure {
  uint32_t struct_size;
  float probability;                   /* chance that an episode has a failure */
  int32_t onset_min, onset_max;        /* control step of the episode at which the rotor fails, inclusive */
  float remaining_min, remaining_max;  /* fraction of its thrust the failed rotor still delivers */
  uint32_t rotor_mask;                 /* bit r: rotor r may fail; 0 = all */
} amenv_rotor_failure;
/* f NULL = off: the handle launches exactly the kernels it launched before. */
int amenv_set_rotor_failure(amenv* env, const amenv_rotor_failure* f);
/* plan [N, 2] int32: the failed rotor (-1: this episode has none) and its onset step (0 with -1); factors [N, n_rotors] f32: the multiplier
 * on s_r in effect for the NEXT step (f on the failed rotor once step >= onset, else 1.0), by the device functions the kernels inline.
 * amenv_dynamics_factors keeps its meaning: the episode's km, kI, s_r, constant within an episode.  Either pointer may be NULL, not both
 * (device memory).  Only enqueues.  Refused while the failure is off. */
int amenv_rotor_failure_state(amenv* env, int32_t* plan, float* factors, void* stream);

/* The part of SB3's PPO.train between the network outputs and the backward pass, fused (three launches instead of ~60 torch
 * kernels): per-minibatch advantage normalisation (mean, unbiased std, eps 1e-8), Gaussian log-prob of `actions` under
 * (mean, log_std), ratio to old_logp, clipped surrogate, value MSE, entropy bonus -- and the gradient of
 *   L = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
 * with respect to mean [n, act_dim], value [n] and log_std [act_dim] (act_dim 4, 5, 6 or 7).  stats4 = {policy_loss, value_loss,
 * entropy_loss, clip_fraction}.  Deterministic (fixed-order reductions, no atomics).  workspace: device buffer of
 * amenv_ppo_workspace_bytes() bytes, 8-byte aligned.  Hyper-parameters of the reference: clip .2, ent 5e-4, vf .5 (v2/rl_train.py:38-53). */
size_t amenv_ppo_workspace_bytes(void);
int amenv_ppo_loss_grad(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                        const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                        float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats4,
                        void* workspace, void* stream);

/* One whole PPO minibatch step of the reference's policy ([128, 64, 64] tanh actor + critic, v2/rl_train.py:27-30,38-53) in ONE fused
 * kernel (+ a launch in front that packs the weights as MFMA operands and a fixed-order reduction behind): forward of both MLPs, SB3's
 * loss as amenv_ppo_loss_grad computes it, backward through both MLPs, all weight / bias gradients.  fp32 in and out on the matrix
 * cores: every operand is split exactly into three bf16 parts (each rounded to nearest) and a product is the sum of the six partial products above 2^-16
 * (v_mfma_f32_32x32x16_bf16, fp32 accumulation; what is dropped is below one fp32 rounding), so the result is as close to the same loss in
 * fp64 as autograd on the fp32 torch modules is (tests/test_gpu_ppo.py).  flat_params / flat_grad: the policy's parameters / their gradients in SB3 state-dict order (see
 * amenv_policy_forward); obs [n, obs_dim], actions [n, act_dim], old_logp / advantages / returns [n] f32; stats4 as amenv_ppo_loss_grad.
 * (obs_dim, act_dim) in {(20,4), (29,7), (17,4), (25,5), (27,6), (24,4), (28,4), (21,4), (25,4)} -- amenv_policy_forward's nine, the last four being the
 * rigid vehicles' rows with action history; any other pair: AMENV_ERR_INVALID, nothing enqueued.  index: NULL, or n row numbers -- minibatch sample s is row index[s] of obs / actions /
 * old_logp / advantages / returns (SB3 draws its minibatches as slices of a permutation of the rollout buffer, RolloutBuffer.get: the
 * gather happens inside the kernel, the rollout tensors stay where they are).  Deterministic: no atomics on the gradient path.
 * workspace: amenv_ppo_mlp_workspace_bytes() bytes, 16-byte aligned. */
size_t amenv_ppo_mlp_workspace_bytes(void);
int amenv_ppo_mlp_step(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                       const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef,
                       float vf_coef, int32_t normalize_advantage, float* flat_grad, float* stats4, void* workspace, void* stream);

/* Gradient-norm clip + Adam on the flat parameter buffer (the torch.nn.utils.clip_grad_norm_ + torch.optim.Adam step of SB3's
 * PPO.train(); Adam with eps 1e-5, v2/rl_train.py:38 through SB3's defaults).  exp_avg / exp_avg_sq / step: torch.optim.Adam's state for
 * that parameter (step: ONE f32 on the device, as torch keeps it with capturable=True; incremented here).  hyper6 (device): lr, beta1,
 * beta2, eps, max_grad_norm (<= 0: no clipping), grad_scale (multiplies the gradient first: 1 / world size after a sum all-reduce).
 * flat_grad (16-byte aligned) is READ-ONLY (the clipped gradient is applied, not stored: every workgroup of the launch takes the norm of the whole buffer
 * as it was on entry), grad_norm_out (may be NULL) receives the norm before clipping.  ticket: one zero-initialised device word the
 * kernel uses and leaves zero. */
int amenv_ppo_adam_step(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, const float* hyper6,
                        float* grad_norm_out, uint32_t* ticket, void* stream);

/* ---- PPO training controls: approx_kl and the on-device target_kl gate -----------------------------------------------
 * SB3 2.6.0 PPO.train computes approx_kl = mean((r - 1) - log r), r = exp(logp - old_logp), per minibatch and, with target_kl set, leaves
 * the update when approx_kl > 1.5 target_kl -- AFTER the loss of that minibatch, BEFORE its optimiser step.  A host-side check would cost
 * one device-to-host synchronisation per minibatch; here the decision is taken and obeyed on the device.
 *
 * amenv_ppo_ctl lives in DEVICE memory, allocated by the caller (amenv_ppo_ctl_bytes() bytes, 4-byte aligned), written by the kernels
 * only, read back by the caller once per update.  amenv_ppo_ctl_arm (one tiny launch, asynchronous on `stream`) sets struct_size and
 * kl_limit and zeroes everything else; call it once per update, before the first minibatch.
 *   - the kernel that finalises a minibatch's scalars (the last launch of amenv_ppo_loss_grad_ctl / amenv_ppo_mlp_step_ctl) adds 1 to
 *     `evaluated`, the minibatch's approx_kl to `kl_sum`, its four scalars to sum[0..3], sets `kl_last`, and sets stop = 1 when
 *     kl_limit > 0 and kl_last > kl_limit (callers pass kl_limit = 1.5 target_kl; <= 0: never stops);
 *   - amenv_ppo_adam_step_ctl with `stop` set changes NOTHING (parameters, both moments, the step counter, grad_norm_out); otherwise the
 *     workgroup that finishes last adds 1 to `applied` and the gradient norm to sum[4];
 *   - every kernel of a later amenv_ppo_loss_grad_ctl / amenv_ppo_mlp_step_ctl call returns at entry while `stop` is set: gradients,
 *     stats and this block keep the values of the minibatch that tripped the limit.
 * With ctl = NULL the three _ctl entry points are the plain ones.  `stats` stays the four floats of the plain entry points with or
 * without ctl: approx_kl of the minibatch is the block's kl_last (read it on the device, or copy the block back).
 * Gradients, parameters and the first four scalars are bit-identical with and without ctl while the gate is open.  Deterministic: every
 * field has one writing thread per launch, sums in fixed order.  One update at a time per block (launches ordered on one stream). */
typedef struct amenv_ppo_ctl {
  uint32_t struct_size; /* = sizeof(amenv_ppo_ctl) = amenv_ppo_ctl_bytes(): guard, written by amenv_ppo_ctl_arm */
  float kl_limit;       /* <= 0: no limit */
  uint32_t stop;        /* 1 once a minibatch's approx_kl exceeded kl_limit */
  uint32_t stop_seen;   /* internal: `stop` as the fused kernel of the current minibatch step read it (what its reduction launch obeys) */
  uint32_t evaluated;   /* minibatches whose loss was computed since the last arm */
  uint32_t applied;     /* Adam steps applied since the last arm */
  float kl_sum;         /* sum of approx_kl over the evaluated minibatches */
  float kl_last;        /* approx_kl of the last evaluated minibatch */
  float sum[5];         /* running sums: policy loss, value loss, entropy loss, clip fraction (evaluated minibatches), grad norm (applied steps) */
  uint32_t reserved[3];
} amenv_ppo_ctl;
size_t amenv_ppo_ctl_bytes(void);
/* AMENV_ERR_INVALID for ctl = NULL or a kl_limit that is NaN */
int amenv_ppo_ctl_arm(amenv_ppo_ctl* ctl, float kl_limit, void* stream);
/* amenv_ppo_loss_grad / amenv_ppo_mlp_step / amenv_ppo_adam_step with the control block as last argument before the stream (NULL: none) */
int amenv_ppo_loss_grad_ctl(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                            const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                            float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats,
                            void* workspace, amenv_ppo_ctl* ctl, void* stream);
int amenv_ppo_mlp_step_ctl(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                           const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef,
                           float vf_coef, int32_t normalize_advantage, float* flat_grad, float* stats, void* workspace, amenv_ppo_ctl* ctl,
                           void* stream);
int amenv_ppo_adam_step_ctl(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, const float* hyper6,
                            float* grad_norm_out, uint32_t* ticket, amenv_ppo_ctl* ctl, void* stream);

/* ---- KL-adaptive learning rate on the device and SB3's clipped value loss ----------------------------------------------
 * The learning rate of the GPU-parallel PPO implementations (rsl_rl, rl_games), driven by every minibatch's approx_kl -- SB3's estimator,
 * the block's kl_last, not the analytic Gaussian KL (the rollout buffer holds no old means).  All in fp32:
 *   if      kl > band * desired_kl:           lr = fmaxf(lr / factor, lr_min)
 *   else if kl > 0 && kl < desired_kl / band: lr = fminf(lr * factor, lr_max)
 *   else                                      lr unchanged                        (a NaN kl: unchanged)
 * A host-side rule would cost one device-to-host synchronisation per minibatch; here the number lives in hyper6[0] and the Adam step moves it.
 *
 * amenv_ppo_lr_rule is a HOST struct, copied into the launch.  amenv_ppo_adam_step_adapt is amenv_ppo_adam_step_ctl with the rule in front of
 * the step -- the order within a minibatch is the gate's: loss -> approx_kl -> rule -> optimiser step, taken with the NEW rate:
 *   - `stop` is tested first: with it set NOTHING changes, hyper6, the step counter and the ticket included;
 *   - otherwise every thread reads hyper6[0] and the block's kl_last at entry and evaluates the rule itself (all agree to the last bit); the
 *     workgroup that finishes last stores the new rate into hyper6[0] (hence non-const); hyper6[1..5] are only read.
 * The rate is NOT in the block: amenv_ppo_ctl keeps its 64 bytes and amenv_ppo_ctl_arm still zeroes all of them.
 * AMENV_ERR_INVALID, nothing enqueued: ctl or rule NULL, rule->struct_size != sizeof(amenv_ppo_lr_rule), a value that is not finite or
 * violates desired_kl > 0, band >= 1, factor > 1, 0 < lr_min <= lr_max, and everything amenv_ppo_adam_step_ctl refuses. */
typedef struct amenv_ppo_lr_rule {
  uint32_t struct_size; /* = sizeof(amenv_ppo_lr_rule): guard, set by the caller */
  float desired_kl;     /* > 0; rsl_rl's default 0.01 */
  float band;           /* >= 1; the rate moves when kl leaves [desired_kl / band, band * desired_kl]; 2 */
  float factor;         /* > 1; 1.5 */
  float lr_min;         /* > 0; 1e-5 */
  float lr_max;         /* >= lr_min; 1e-2 */
} amenv_ppo_lr_rule;
int amenv_ppo_adam_step_adapt(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, float* hyper6,
                              float* grad_norm_out, uint32_t* ticket, amenv_ppo_ctl* ctl, const amenv_ppo_lr_rule* rule, void* stream);

/* SB3 2.6.0's clipped value loss (clip_range_vf): v_pred = v_old + clamp(v - v_old, -c, c), value_loss = mean((returns - v_pred)^2); the gradient
 * passes where -c <= v - v_old <= c (torch.clamp's backward).  The two entry points take the _ctl argument lists plus old_values [n] f32
 * (gathered through `index` like old_logp) and clip_range_vf (> 0 and finite, else AMENV_ERR_INVALID; old_values NULL likewise) in front of the
 * stream; ctl may be NULL.  They launch a third form of the loss kernels; every other kernel of the step is the _ctl (ctl given) or the plain
 * (ctl NULL) one.  An unclipped sample enters with v itself: with clip_range_vf above every |v - v_old| the results are the _ctl entry
 * points' bit for bit. */
int amenv_ppo_loss_grad_vclip(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                              const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                              float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats,
                              void* workspace, amenv_ppo_ctl* ctl, const float* old_values, float clip_range_vf, void* stream);
int amenv_ppo_mlp_step_vclip(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                             const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef,
                             float vf_coef, int32_t normalize_advantage, float* flat_grad, float* stats, void* workspace, amenv_ppo_ctl* ctl,
                             const float* old_values, float clip_range_vf, void* stream);

/* Parity gate of the arm vehicle's arithmetic (no reference dynamics exist for it; DESIGN.md "arm"): the 19 state derivatives of n states
 * [n, 19] = (p, v, q, w, th, thd) under post-mixer wrenches [n, 4] = (F, Mx, My, Mz) and joint commands [n, 3], deriv [n, 19], all of `dtype`
 * (AMENV_F32 | AMENV_F64), on the current device.  form 0: the per-link Newton-Euler sums the lane and two-wave kernels run; form 1: the staged
 * form (joint-configuration aggregates, then the base dynamics on them) the stage-wave and lane-team kernels run.  Tests compare both fp64
 * instantiations with the oracle's right-hand side (<= 1e-12).  cfg: an arm vehicle with the z,x,x joint axes. */
int amenv_arm_rhs(const amenv_config* cfg, int32_t form, int32_t dtype, const void* state19, const void* wrench4, const void* cmd3, void* deriv19,
                  int64_t n, void* stream);

/* ---- PID + minimum-snap baseline controller ------------------------------------------------------------
 * The reference's hand-tuned controller, `v2/PID Controller/{pid_controller,trajGen3D,runsim}.py`, for N vehicles per launch on caller-owned
 * device buffers of the CURRENT device.  `dtype` selects the arithmetic of the float buffers marked (dtype): AMENV_F64 = the logic gate
 * pinned to the reference's recorded run (tests/golden/pid_helix.npz), AMENV_F32 = the product build. */
typedef struct amenv_pid_params {
  double dt;           /* control period the integrals are advanced by (runsim.py:28: 0.01; the waypoint env: 1/200) */
  double mass, g;      /* params.py:10-11 */
  double max_integral; /* pid_controller.py:34: 100 */
  double gain[18];     /* [x, y, z, phi, theta, psi][k_p, k_d, k_i]  (pid_controller.py:16-21) */
} amenv_pid_params;
/* The committed gains and the reference quadrotor's mass / g; dt = 0.01. */
int amenv_pid_default_params(amenv_pid_params* p);

/* pid_controller.run (pid_controller.py:37-115) with Quadcopter.attitude() (model/quadcopter.py:57-59):
 *   state    [n, 13] (dtype) position, velocity, quaternion (w, x, y, z), body rates = Quadcopter.state
 *   des      [n, 11] (dtype) desired position, velocity, acceleration, yaw, yaw rate  (trajGen3D.DesiredState)
 *   integral [n, 6]  (dtype) in/out: the module's integral memory (x, y, z, phi, theta, psi), clamped to +-max_integral
 *   F_out [n], M_out [n, 3] (dtype): thrust and moments BEFORE the mixer;  rpy_out [n, 3] (dtype) or NULL: the attitude it used */
int amenv_pid_run(const amenv_pid_params* p, int32_t dtype, const void* state, const void* des, void* integral, void* F_out, void* M_out,
                  void* rpy_out, int64_t n, void* stream);

/* trajGen3D.get_MST_coefficients / MST (:211-292) for n_traj trajectories of n_segments (1..16) 7th-order segments each:
 *   waypoints [n_traj, n_segments + 1, 3] f64  ->  coeff [n_traj, 8 n_segments, 3] f64 (the reference's coeff_x / _y / _z as columns),
 *   seg_time [n_traj, n_segments] = |w_i - w_i+1| / speed and seg_start [n_traj, n_segments + 1] = their running sum (:97-103).
 * The 8n x 8n constraint matrix depends on n_segments only: it is inverted on the device (fp64 Gauss-Jordan, partial pivoting) into
 * `workspace` (amenv_minsnap_workspace_bytes(n_segments) bytes, 8-byte aligned), then every trajectory is one small matrix product. */
size_t amenv_minsnap_workspace_bytes(int32_t n_segments);
int amenv_minsnap_solve(int32_t n_segments, int64_t n_traj, double speed, const double* waypoints, double* coeff, double* seg_time,
                        double* seg_start, void* workspace, void* stream);
/* trajGen3D.generate_trajectory (:76-187) for n_query (trajectory, time) pairs: query i evaluates trajectory traj[i] (traj NULL: i)
 * at t[i] (f64) -> des [n_query, 11] (dtype): position, velocity, acceleration, yaw = yaw rate = 0 (:183-184); t == 0 returns the first
 * waypoint at rest (:108-111), t past the last segment the last waypoint at rest (:121,176-179). */
int amenv_minsnap_eval(int32_t n_segments, int64_t n_query, const double* coeff, const double* seg_time, const double* seg_start,
                       const double* waypoints, const int64_t* traj, const double* t, int32_t dtype, void* des, void* stream);

/* The controller wired to the waypoint environment as a closed-loop action source (the way runsim.py:26-31 flies its waypoint list):
 * per episode a ONE-segment rest-to-rest minimum-snap trajectory from where the episode started to the waypoint at `speed` m/s, tracked
 * by the PID; thrust scaled by mass, moments by inertia_ratio (this vehicle's inertia / the reference quadrotor's, per axis) and the
 * moment vector scaled into the action box.  One launch: observation rows in, action rows out.
 *   obs     [n, obs_dim] f32, v2 layout (rl_env_scaledObs.py:98-121), obs_dim >= 20 (23 + 2 n with an n-link arm)
 *   done    [n] u8 or NULL: envs whose episode ended on the previous step (auto-reset => a new trajectory starts)
 *   pstate  [n, 14] (dtype) in/out: t, start (3), goal (3), integrals (6), fresh; initialise to {0 x 13, 1}
 *   actions [n, act_dim] f32, act_dim >= 4: thrust / (m g) in [0, 2], moments in [-1, 1]; entries 4.. (arm joints) = 0 (home)
 * tool_mode = 1 (arm vehicle with AMENV_EE_TASK_TOOL, obs_dim >= 23): the position loop tracks the tool point instead of the base; the
 * tool offset is read from the LAST three columns of the row (26..28 for the 3-link arm, 22..24 / 24..26 for 1 / 2 links). */
typedef struct amenv_pid_policy_params {
  amenv_pid_params pid;
  double speed;            /* m/s along the segment (runsim.py:27 flies 1.2) */
  double moment_scale;     /* amenv_vehicle.moment_scale */
  double inertia_ratio[3];
  int32_t obs_dim, act_dim, tool_mode, reserved;
} amenv_pid_policy_params;
int amenv_pid_policy(const amenv_pid_policy_params* p, int32_t dtype, const float* obs, const uint8_t* done, void* pstate, float* actions,
                     int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMENV_H_ */
