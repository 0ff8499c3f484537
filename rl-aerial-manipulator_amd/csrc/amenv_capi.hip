// amenv_capi.hip -- core source of libamenv.so's host side, the C ABI declared in include/amenv.h: env lifecycle and switches, reset /
// observe / state, the two normalisers, the PID / min-snap baseline, and the functions amenv_host.hpp declares for the other sources
// (amenv_capi_step / _rollout / _policy / _policy_norm / _eval / _train.hip: DESIGN 4x).
// Owns the SoA episode state on one device, validates arguments, picks the kernel
// instantiation (arithmetic type x rotor count x workgroup size) and enqueues it on the
// caller's stream.  No synchronisation and no allocation after amenv_create().
#include "amenv_host.hpp"
#include "amenv_policy_pack.hpp"
#include "amenv_obsnorm_kernels.hpp"
#include "amenv_retnorm.hpp"
#include "amenv_baseline.hpp"

static thread_local std::string g_create_err;

int fail(amenv* e, int code, const std::string& msg) {
  if (e) e->err = msg; else g_create_err = msg;
  return code;
}

namespace {

constexpr int kStatsWords = kStampBase + kStampWaves * kStampSlots;  // totals + diagnostic stamp area

// small dense helpers (host, fp64) for the default vehicles
bool invert(int n, const double* a, double* out) {  // Gauss-Jordan, partial pivoting, n <= 4
  double m[4][8];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) { m[i][j] = a[i * n + j]; m[i][n + j] = (i == j) ? 1.0 : 0.0; }
  for (int c = 0; c < n; c++) {
    int p = c;
    for (int r = c + 1; r < n; r++) if (std::fabs(m[r][c]) > std::fabs(m[p][c])) p = r;
    if (std::fabs(m[p][c]) < 1e-300) return false;
    if (p != c) for (int j = 0; j < 2 * n; j++) std::swap(m[c][j], m[p][j]);
    const double d = m[c][c];
    for (int j = 0; j < 2 * n; j++) m[c][j] /= d;
    for (int r = 0; r < n; r++) if (r != c) { const double f = m[r][c]; for (int j = 0; j < 2 * n; j++) m[r][j] -= f * m[c][j]; }
  }
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) out[i * n + j] = m[i][n + j];
  return true;
}

// alloc = A^T (A A^T)^-1  (right pseudo-inverse of the 4 x n mixer; = A^-1 for n = 4)
bool allocation_from_mix(int n, const double* A /*[4][n]*/, double* alloc /*[n][4]*/) {
  double G[16], Gi[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) { double s = 0; for (int r = 0; r < n; r++) s += A[i * n + r] * A[j * n + r]; G[i * 4 + j] = s; }
  if (!invert(4, G, Gi)) return false;
  for (int r = 0; r < n; r++)
    for (int j = 0; j < 4; j++) { double s = 0; for (int i = 0; i < 4; i++) s += A[i * n + r] * Gi[i * 4 + j]; alloc[r * 4 + j] = s; }
  return true;
}

void fill_task_defaults(amenv_task* t, int K) {
  t->variant = AMENV_TASK_V2_SCALED20;
  t->num_waypoints = K;          // rl_env_scaledObs.py:47
  t->max_episode_steps = 2000;   // :56
  t->counter_limit = 500;        // :59
  t->rk4_substeps = 1;
  t->ee_task = AMENV_EE_TASK_BASE;
  t->dt = 1.0 / 200.0;           // :30
  const double pi = 3.14159265358979323846;
  for (int k = 1; k <= K; k++) {
    const double tt = double(k) / double(K);
    t->traj_sin[k - 1] = std::sin(2.0 * tt * pi);   // utils2/utils.py:39
    t->traj_cos[k - 1] = std::cos(tt * 2.0 * pi);   // utils2/utils.py:83-86
  }
}

// the reference's 0.18 kg quadrotor: v2/simul_files/model/params.py:10-36
bool vehicle_quad(amenv_vehicle* v) {
  v->n_rotors = 4; v->n_joints = 0;
  v->mass = 0.18; v->g = 9.81;
  const double I[9] = {0.00025, 0, 2.55e-6, 0, 0.000232, 0, 2.55e-6, 0, 0.0003738};
  std::memcpy(v->inertia, I, sizeof(I));
  if (!invert(3, I, v->inv_inertia)) return false;
  const double L = 0.086, r = 1.5e-9 / 6.11e-8;
  const double A[16] = {1, 1, 1, 1, 0, L, 0, -L, -L, 0, L, 0, r, -r, r, -r};
  std::memcpy(v->mix, A, sizeof(A));
  if (!invert(4, A, v->alloc)) return false;
  const double maxF = 2.0 * v->mass * v->g, minF = 0.0;
  for (int i = 0; i < 4; i++) { v->t_min[i] = minF / 4; v->t_max[i] = maxF / 4; }
  v->moment_scale = 0.1;  // rl_env_scaledObs.py:126
  return true;
}

// The repo's 6-rotor airframe (hexacopter_description/custom_hexa/model.sdf + airframe/4022_*):
// no reference dynamics code exists for it -> parity unpinned; constants derived in DESIGN.md "hexa".
bool vehicle_hexa(amenv_vehicle* v) {
  v->n_rotors = 6; v->n_joints = 0;
  v->mass = 2.7211; v->g = 9.81;
  // composite inertia about the CoG: 27 SDF links composed with the parallel-axis theorem by
  // tools/hexa_params.py (total 2.7211 kg, CoG z = 0.04122 m; off-diagonals < 1e-14 dropped)
  const double I[9] = {4.4024422324e-02, 0, 0, 0, 4.4059346318e-02, 0, 0, 0, 7.7083344191e-02};
  std::memcpy(v->inertia, I, sizeof(I));
  if (!invert(3, I, v->inv_inertia)) return false;
  // rotor positions (FLU, m) and spin (custom_hexa_arm/model.sdf:653,769,882,995,1108,1221; plugins :1631-1733)
  const double x[6] = {-0.255691, 0.255691, -0.255691, 0.255691, 0.0, 0.0};
  const double y[6] = {0.1475, -0.1475, -0.1475, 0.1475, 0.295, -0.295};
  const double sg[6] = {+1, -1, -1, +1, -1, +1};  // +1 cw, -1 ccw (reaction torque sign in z-up)
  const double mc = 0.0168;                       // moment constant, m
  double A[4 * 6];
  for (int r = 0; r < 6; r++) { A[0 * 6 + r] = 1.0; A[1 * 6 + r] = y[r]; A[2 * 6 + r] = -x[r]; A[3 * 6 + r] = sg[r] * mc; }
  std::memcpy(v->mix, A, sizeof(A));
  if (!allocation_from_mix(6, A, v->alloc)) return false;
  const double kf = 2.11e-5;  // N/(rad/s)^2 ; speed limits 150..820 rad/s (airframe/4022_*:64-76)
  for (int r = 0; r < 6; r++) { v->t_min[r] = kf * 150.0 * 150.0; v->t_max[r] = kf * 820.0 * 820.0; }
  v->moment_scale = 1.0;  // free parameter (no reference value): +-1 action = +-1 N m
  return true;
}

// BASELINE config 3: the hexacopter carrying the 3-joint arm (custom_hexa_arm/model.sdf:1741-1759 attaches
// Manipulator/.../sdf/manipulator.sdf to base_link).  All numbers printed by tools/arm_params.py from those SDF files.
// Parity unpinned (no reference dynamics); servo gains are this build's choice (DESIGN.md "arm").
bool vehicle_hexa_arm(amenv_vehicle* v) {
  if (!vehicle_hexa(v)) return false;
  v->n_joints = 3;
  v->mass = 3.2121;  // total: base body 2.8561 (27 hexacopter links + base_plate lump) + links 0.082 + 0.054 + 0.220
  // base body inertia about its own CoM (= body-frame origin O; model-frame z = 0.038523)
  const double I[9] = {4.4499781211e-02, 0, 8.3146456634e-06, 0, 4.4545235795e-02, 0, 8.3146456634e-06, 0, 7.7122576031e-02};
  std::memcpy(v->inertia, I, sizeof(I));
  if (!invert(3, I, v->inv_inertia)) return false;
  const double jo[9] = {0.0094667379, -0.01, -0.103522586,   // joint_1 in the body frame (manipulator.sdf:99, rel. O)
                        0.0, 0.0125, 0.0,                     // joint_2 in link 1 (:159)
                        0.0, 0.0, -0.106};                    // joint_3 in link 2 (:233)
  const double ja[9] = {0, 0, 1, 1, 0, 0, 1, 0, 0};          // axes z, x, x (:103,163,237)
  const double lm[3] = {0.082, 0.054, 0.220};                // :131,191,265 (+ 2 x 0.02 closed gripper fingers in link 3)
  const double lc[9] = {0, 0, 0, 0, 0, -0.052, 0.0058295455, -0.0054545455, -0.0822272727};
  const double li[27] = {2.10193333e-05, 0, 0, 0, 2.31308333e-05, 0, 0, 0, 3.62781667e-05,
                         1.980045e-04, 0, 0, 0, 2.266425e-04, 0, 0, 0, 3.4263e-05,
                         8.2716818176e-04, 2.6844545455e-05, 5.7916022727e-05, 2.6844545455e-05, 8.5215807772e-04, -5.1327272727e-05,
                         5.7916022727e-05, -5.1327272727e-05, 1.0384565341e-04};
  std::memcpy(v->joint_origin, jo, sizeof(jo)); std::memcpy(v->joint_axis, ja, sizeof(ja));
  std::memcpy(v->link_mass, lm, sizeof(lm)); std::memcpy(v->link_com, lc, sizeof(lc)); std::memcpy(v->link_inertia, li, sizeof(li));
  v->joint_kp = 100.0; v->joint_kd = 20.0;   // critically damped position servo, 10 rad/s bandwidth (this build's choice)
  v->joint_acc_max = 8.0;                    // manipulator_moveit/config/joint_limits.yaml:9-51
  v->joint_reserved = 0.0;
  const double lim[6] = {-3.14, 3.14, -1.57, 1.57, -1.57, 1.57};   // manipulator.sdf:105-106,165-166,239-240
  std::memcpy(v->joint_limit, lim, sizeof(lim));
  const double tool[3] = {-0.0015, 0.003, -0.125};   // midpoint of the gripper-finger joint origins in link 3's frame (manipulator.sdf:371,450)
  std::memcpy(v->tool_offset, tool, sizeof(tool));
  return true;
}

// the per-lane table on the device (float4 pieces for fp32, plain doubles for the fp64 build); with_params: the team kernels' parameters
// behind it (the step kernel's source; the other team kernels take them as arguments)
template <typename T> hipError_t upload_team_consts(amenv* e, bool with_params) {
  const std::vector<T> tc = team_const_table<T>(e->cfg, sizeof(T) == 4);
  hipError_t s;
  if ((s = hipMalloc(&e->team_consts, with_params ? team_block_bytes<T>() : tc.size() * sizeof(T))) != hipSuccess ||
      (s = hipMemcpy(e->team_consts, tc.data(), tc.size() * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess)
    return s;
  if (!with_params) return hipSuccess;
  const TeamParamsT<T> P = make_team<T>(*e);
  return hipMemcpy(static_cast<char*>(e->team_consts) + team_table_bytes<T>(), &P, sizeof(P), hipMemcpyHostToDevice);
}

// episode-start rotor state: the rotors spin at the NOMINAL hover command, sqrt(clamp(alloc[r] . (m g, 0, 0, 0))), fp64
double lag_w0(const amenv_vehicle& v, int r) {
  const double t = v.alloc[r * 4] * (v.mass * v.g);
  return std::sqrt(std::fmax(std::fmin(t, v.t_max[r]), v.t_min[r]));
}

int obs_dim_of(const amenv_config* c) { return is_v1(c) ? 17 : 20 + 2 * c->vehicle.n_joints + (c->vehicle.n_joints ? 3 : 0); }
int act_dim_of(const amenv_config* c) { return kActDim + c->vehicle.n_joints; }

int n_float_fields(const amenv_config* c) { return AMENV_F_WP0 + 3 * c->task.num_waypoints + 2 * c->vehicle.n_joints; }

const char* validate(const amenv_config* c) {
  if (!c) return "config is NULL";
  if (c->struct_size != sizeof(amenv_config)) return "amenv_config.struct_size mismatch (ABI)";
  if (c->abi_version != AMENV_ABI_VERSION) return "amenv_config.abi_version mismatch";
  if (c->num_envs <= 0) return "num_envs must be > 0";
  if (c->dtype != AMENV_F32 && c->dtype != AMENV_F64) return "dtype must be AMENV_F32 or AMENV_F64";
  if (c->vehicle.n_rotors < 1 || c->vehicle.n_rotors > AMENV_MAX_ROTORS) return "n_rotors out of range";
  if (c->vehicle.n_joints < 0 || c->vehicle.n_joints > AMENV_MAX_JOINTS) return "n_joints must be 0..3";
  if (c->vehicle.n_joints > 0 && (c->vehicle.n_rotors != 6 || is_v1(c)))
    return "arm vehicles are built for the 6-rotor airframe and the v2 task (BASELINE config 3; 1 waypoint on every kernel, 2..4 on the lane kernel)";
  if (c->task.variant != AMENV_TASK_V2_SCALED20 && !is_v1(c)) return "unknown task variant";
  if (is_v1(c) && c->task.num_waypoints > 2) return "v1 tasks draw 1..2 waypoints per episode: num_waypoints (storage bound) must be 1 or 2";
  if (c->task.num_waypoints < 1 || c->task.num_waypoints > AMENV_MAX_WAYPOINTS) return "num_waypoints out of range";
  if (c->task.max_episode_steps < 1 || c->task.counter_limit < 0) return "bad episode limits";
  if (c->task.rk4_substeps < 0 || c->task.rk4_substeps > 64) return "rk4_substeps out of range";
  if (!(c->task.dt > 0.0) || !(c->vehicle.mass > 0.0)) return "dt and mass must be positive";
  for (int r = 0; r < c->vehicle.n_rotors; r++)
    if (std::fabs(c->vehicle.mix[r] - 1.0) > 1e-12) return "mix row 0 must be all ones: total thrust is the plain sum of rotor thrusts (quadcopter.py:111)";
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < i; j++)
      if (std::fabs(c->vehicle.inertia[i * 3 + j] - c->vehicle.inertia[j * 3 + i]) > 1e-15 ||
          std::fabs(c->vehicle.inv_inertia[i * 3 + j] - c->vehicle.inv_inertia[j * 3 + i]) > 1e-6 * std::fabs(c->vehicle.inv_inertia[i * 3 + i]))
        return "inertia and inv_inertia must be symmetric";
  // the blob holds whole 256-lane groups of tiles and padding lanes run unguarded: the workgroup size must divide 256
  if (c->block_size != 0 && c->block_size != 64 && c->block_size != 128 && c->block_size != 256) return "block_size must be 0, 64, 128 or 256";
  if (c->step_kernel < AMENV_KERNEL_AUTO || c->step_kernel > AMENV_KERNEL_STAGED) return "unknown step_kernel";
  if (c->task.ee_task != AMENV_EE_TASK_BASE && c->task.ee_task != AMENV_EE_TASK_TOOL) return "unknown task.ee_task";
  return nullptr;
}

constexpr int kTeamAutoMax = 6144;    // AUTO: lane-team kernel up to this batch
constexpr int kArmkAutoMax = 32768;   // AUTO: stage-wave kernel up to this batch

}  // namespace

// Which step kernel a config runs: amenv_config.step_kernel, or by batch size for AUTO (crossovers measured on MI355X).
// Returns the refusal text when a requested kernel is not built for the config.
const char* select_step_family(const amenv_config& c, StepFamily* out) {
  const int want = c.step_kernel, n = c.num_envs;
  const bool autok = want == AMENV_KERNEL_AUTO, f32 = c.dtype == AMENV_F32, arm = zxx_arm1(c);
  StepFamily f = StepFamily::Lane;
  // team vs stage-wave kernel: 5.96 vs 6.98 us at 6144 envs, 7.04 vs 6.99 at 7168 (profiles/r03/crossover_team_vs_stage_wave.txt)
  if (arm && (want == AMENV_KERNEL_TEAM || (f32 && autok && n <= kTeamAutoMax)))
    f = StepFamily::Team;
  // stage-wave vs two-wave kernel: 9.3 vs 10.6 us at 32768 envs, behind from 53248; built for one RK4 sub-step (rk4_substeps = 1 only)
  else if (arm && c.task.rk4_substeps == 1 && (want == AMENV_KERNEL_STAGED || (f32 && autok && n > kTeamAutoMax && n <= kArmkAutoMax)))
    f = StepFamily::Staged;
  // two-wave vs lane kernel: still ahead at 65536 envs, 18.0 vs 19.5 us
  else if (arm && f32 && (want == AMENV_KERNEL_HELPER || (autok && n <= 65536)))
    f = StepFamily::TwoWave;
  // lane-quad kernel: opt-in only, it ties with the helper-wave kernel at small batches and loses above (profiles/r02/crossover_quad_vs_pw.txt)
  else if (quad_ok(c) && want == AMENV_KERNEL_TEAM)
    f = StepFamily::Quad;
  // helper waves pay while the launch is latency-bound; the Monitor wave owns one of the kStatsReplicas replicas per tile
  else if (c.vehicle.n_joints == 0 && c.block_size == 0 && (autok ? n <= 32768 : want == AMENV_KERNEL_HELPER && n <= 64 * kStatsReplicas))
    f = StepFamily::LaneHelper;
  if (f == StepFamily::Lane && want == AMENV_KERNEL_HELPER)
    return "AMENV_KERNEL_HELPER is built for fp32 z,x,x-arm vehicles and for rigid vehicles with block_size = 0 "
           "and at most 65536 envs (its Monitor wave owns one of the 1024 replicas of the running totals per tile)";
  if (f == StepFamily::Lane && want == AMENV_KERNEL_TEAM)
    return "AMENV_KERNEL_TEAM is built for the 6-rotor vehicle with the z,x,x arm (16 lanes per env; fp64 = logic-gate build) and for "
           "fp32 rigid vehicles with 4 or 6 rotors, the single-waypoint v2 task and block_size = 0 (4 lanes per env)";
  if (f == StepFamily::Lane && want == AMENV_KERNEL_STAGED)
    return "AMENV_KERNEL_STAGED is built for the 6-rotor vehicle with the z,x,x arm (fp64 = logic-gate build), the single-waypoint v2 task "
           "and rk4_substeps = 1";
  *out = f;
  return nullptr;
}

// Lane-team step kernel: four integrating waves + one helper per workgroup while every workgroup gets a CU to itself, else one + one
// (amenv_team.hpp, step_kernel_team).
bool team_wide(const amenv& e) {
  static std::mutex m;
  static int cus[64] = {0};
  const int d = e.device >= 0 && e.device < 64 ? e.device : 0;
  std::lock_guard<std::mutex> g(m);
  if (cus[d] == 0) {
    int v = 0;
    cus[d] = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && v > 0 ? v : 1;
  }
  return e.n_tiles * 4 <= cus[d];
}

// amenv_kernel_name: tests, tools/ and bench.py match substrings of it
std::string kernel_name(const amenv& e) {
  const amenv_config& c = e.cfg;
  const char* t = c.dtype == AMENV_F64 ? "double" : "float";
  const int nrot = (c.vehicle.n_rotors == 4 || c.vehicle.n_rotors == 6) ? c.vehicle.n_rotors : AMENV_MAX_ROTORS;
  const int kw = is_v1(&c) ? 2 : (c.task.num_waypoints == 1 ? 1 : AMENV_MAX_WAYPOINTS);
  char buf[200] = "";
  switch (e.family) {
    case StepFamily::Lane:
      std::snprintf(buf, sizeof(buf), "step_kernel<%s,NROT=%d,KW=%d,%s> block=%d", t, nrot, kw, c.vehicle.n_joints ? "v2+arm3" : (is_v1(&c) ? "v1" : "v2"), e.block); break;
    case StepFamily::LaneHelper:
      std::snprintf(buf, sizeof(buf), "step_kernel_pw<%s,NROT=%d,KW=%d,%s> (main wave + reset wave [+ observation wave + Monitor wave] per 64-env tile)", t, nrot, kw,
                    is_v1(&c) ? "v1" : "v2"); break;
    case StepFamily::Quad:
      std::snprintf(buf, sizeof(buf), "step_kernel_quad<NROT=%d,v2> (4 lanes per env, 16 envs per wave + episode-end helper wave)", c.vehicle.n_rotors); break;
    case StepFamily::Team:
      std::snprintf(buf, sizeof(buf), "step_kernel_team<%s,NROT=6,v2+arm3> (16 lanes per env: 4 RK4 stages x 4 components, 4 envs per wave + %s)", t,
                    team_wide(e) ? "one episode-end helper wave per 4" : "episode-end helper wave"); break;
    case StepFamily::Staged:
      std::snprintf(buf, sizeof(buf), "step_kernel_armk<%s,NROT=6> block=320 (4 RK4 stage waves + main wave per 64-env tile)", t); break;
    case StepFamily::TwoWave:
      std::snprintf(buf, sizeof(buf), "step_kernel_arm2w<float,NROT=6> block=128 (2 waves per 64-env tile)"); break;
  }
  std::string name = buf;
  if (e.dr) name += " +dr";
  if (e.lag) name += " +lag";
  if (e.noise) name += " +noise";
  if (e.delay) name += " +delay";
  if (e.hist) name += " +history " + std::to_string(e.hist);
  if (e.rate.on) name += " +rate";
  if (e.fail.ctl) name += " +fail";
  if (e.pub_nj == 1 || e.pub_nj == 2) name += " [" + std::to_string(e.pub_nj) + "-joint arm: phantom links inside, pack / unpack at the C ABI]";
  return name;
}

namespace {

template <typename T>
hipError_t launch_reset(const amenv& e, const uint8_t* mask, float* obs, int pad_only, hipStream_t s) {
  const int bs = 256, n_pad = e.n_tiles * 64;
  hipLaunchKernelGGL((reset_kernel<T>), dim3((n_pad + bs - 1) / bs), dim3(bs), 0, s, e.cfg.num_envs, n_pad, e.cfg.task.num_waypoints, e.cfg.task.variant, e.cfg.vehicle.n_joints,
                     e.cfg.task.ee_task, e.tile_bytes, make_cold(e), make_arm<T>(e), e.blob, mask, obs, pad_only, make_noise_rt(e));
  return hipGetLastError();
}
hipError_t launch_reset(const amenv& e, const uint8_t* mask, float* obs, int pad_only, hipStream_t s) { return e.cfg.dtype == AMENV_F64 ? launch_reset<double>(e, mask, obs, pad_only, s) : launch_reset<float>(e, mask, obs, pad_only, s); }

template <typename T>
hipError_t launch_observe(const amenv& e, float* obs, float* ee, hipStream_t s) {
  const int n = e.cfg.num_envs, bs = 256, K = e.cfg.task.num_waypoints, nj = e.cfg.vehicle.n_joints;
  if (obs) hipLaunchKernelGGL((observe_kernel<T>), dim3((n + bs - 1) / bs), dim3(bs), 0, s, n, K, e.cfg.task.variant, nj, e.cfg.task.ee_task, e.tile_bytes, make_arm<T>(e),
                              (const void*)e.blob, obs, make_noise_rt(e));
  if (ee) hipLaunchKernelGGL((ee_position_kernel<T>), dim3((n + bs - 1) / bs), dim3(bs), 0, s, n, K, nj, e.tile_bytes, make_arm<T>(e), (const void*)e.blob, ee);
  return hipGetLastError();
}
hipError_t launch_observe(const amenv& e, float* obs, float* ee, hipStream_t s) { return e.cfg.dtype == AMENV_F64 ? launch_observe<double>(e, obs, ee, s) : launch_observe<float>(e, obs, ee, s); }

template <typename T>
hipError_t launch_transpose(const amenv& e, void* f, int32_t* i, int to_api, hipStream_t s) {
  const int bs = 256, n = e.cfg.num_envs;
  hipLaunchKernelGGL((transpose_state_kernel<T>), dim3((n + bs - 1) / bs), dim3(bs), 0, s, n, e.nf, e.cfg.task.num_waypoints, e.pub_nj /* the caller's joint fields: th[0..n), thd[0..n) */, e.tile_bytes, e.blob, (T*)f, i, to_api);
  return hipGetLastError();
}
hipError_t launch_transpose(const amenv& e, void* f, int32_t* i, int to_api, hipStream_t s) { return e.cfg.dtype == AMENV_F64 ? launch_transpose<double>(e, f, i, to_api, s) : launch_transpose<float>(e, f, i, to_api, s); }

// amenv_dynamics_factors: [N][2 + NROT] = km, kI, s_0.. of every env's current episode (dr_draw: the kernels' own arithmetic)
template <int NROT>
__global__ void dr_factors_kernel(int n, uint32_t tile_bytes, const void* __restrict__ blob, const ColdParams C, const DrRanges R, float* __restrict__ out) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int32_t episode = iptr4(const_cast<char*>(tile_base(blob, tile_bytes, i)), i & 63)->w;
  float f[2 + NROT];
  dr_draw<NROT>(C, R, C.gid0 + i, episode, f);
#pragma unroll
  for (int k = 0; k < 2 + NROT; k++) out[size_t(i) * (2 + NROT) + k] = f[k];
}

// amenv_rate_moment_actions: [N][4] = the thrust entry, then the moment action the rate loop forms from the given commands and every env's current
// body rates (rate_to_moment: the kernels' own arithmetic)
template <int NROT>
__global__ void rate_moment_kernel(int n, uint32_t tile_bytes, const void* __restrict__ blob, const HotParams<float, NROT> P, const RateBlock Q,
                                   const float4* __restrict__ actions, float4* __restrict__ out) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const Vec4<float> w = *gptr<float>(const_cast<char*>(tile_base(blob, tile_bytes, i)), i & 63, 3);   // {wx, wy, wz, ep_return}
  const float4 a = actions[i];
  float act[4] = {a.x, a.y, a.z, a.w};
  rate_to_moment(P, Q, w.a, w.b, w.c, act);
  out[i] = make_float4(act[0], act[1], act[2], act[3]);
}

// amenv_rotor_failure_state: plan [N][2] = the rotor (-1: none) and the onset of every env's current episode, factors [N][NROT] = the multiplier
// on s_r in effect for the NEXT step (fail_draw and fail_hit: the kernels' own draw and compare, on a row of ones)
template <int NROT>
__global__ void fail_state_kernel(int n, uint32_t tile_bytes, const void* __restrict__ blob, const ColdParams C, const FailBlock X, int32_t* __restrict__ plan,
                                  float* __restrict__ factors) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int4 iv = *iptr4(const_cast<char*>(tile_base(blob, tile_bytes, i)), i & 63);   // {step, counter, flags, episode}
  FailLane fl = fail_draw<NROT>(C, X, C.gid0 + i, iv.w);
  if (plan) { plan[2 * size_t(i)] = fl.key >= 0 ? fl.key >> 16 : -1; plan[2 * size_t(i) + 1] = fl.key >= 0 ? fl.key & 0xffff : 0; }
  float s[NROT];
#pragma unroll
  for (int r = 0; r < NROT; r++) s[r] = 1.0f;
  fail_hit<float, NROT>(fl, iv.x, s);
  if (factors) {
#pragma unroll
    for (int r = 0; r < NROT; r++) factors[size_t(i) * NROT + r] = s[r];
  }
}

// amenv_sensor_noise_samples: [N][12] = the twelve unit samples of every env's current (episode, step) (noise_block: the kernels' own draw)
__global__ void noise_samples_kernel(int n, uint32_t tile_bytes, const void* __restrict__ blob, const ColdParams C, float* __restrict__ out) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int4 iv = *iptr4(const_cast<char*>(tile_base(blob, tile_bytes, i)), i & 63);   // {step, counter, flags, episode}
#pragma unroll
  for (uint32_t b = 0; b < 3; b++) {
    float f[4];
    noise_block(C.seed_lo, C.seed_hi, C.gid0 + i, iv.w, iv.x, b, f);
#pragma unroll
    for (int k = 0; k < 4; k++) out[size_t(i) * 12 + 4 * b + k] = f[k];
  }
}

// amenv_set_rotor_lag / amenv_reset: w <- w0 for the masked envs (mask null = all; padding lanes always, as reset_kernel does)
template <typename T, int NROT>
__global__ void lag_reset_kernel(int n, const LagArg<T, NROT, true> L, const uint8_t* __restrict__ mask) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= int(L.n_pad)) return;
  if (i < n && mask && !mask[i]) return;
#pragma unroll
  for (int r = 0; r < NROT; r++) L.w[lag_slot<NROT>(i) + r * 64] = L.w[size_t(NROT) * L.n_pad + r];
}
// amenv_get_rotor_state (to_api) / amenv_set_rotor_state: [N][NROT] row-major <-> the side buffer's [tile][NROT][64]
template <typename T>
__global__ void lag_transpose_kernel(int n, int nr, T* __restrict__ w, T* __restrict__ api, int to_api) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  T* p = w + size_t(i >> 6) * (nr * 64) + size_t(i & 63);
  for (int r = 0; r < nr; r++) {
    if (to_api) api[size_t(i) * nr + r] = p[r * 64];
    else p[r * 64] = api[size_t(i) * nr + r];
  }
}
template <typename T>
hipError_t launch_lag_reset(const amenv& e, const uint8_t* mask, hipStream_t s) {
  const int n = e.cfg.num_envs;
  const dim3 grid(e.n_tiles / 4), block(256);
  with_rotors46(e.cfg.vehicle.n_rotors, [&](auto nrot) {
    hipLaunchKernelGGL((lag_reset_kernel<T, decltype(nrot)::value>), grid, block, 0, s, n, make_lag<T, decltype(nrot)::value>(e), mask);
  });
  return hipGetLastError();
}
hipError_t launch_lag_reset(const amenv& e, const uint8_t* mask, hipStream_t s) { return e.cfg.dtype == AMENV_F64 ? launch_lag_reset<double>(e, mask, s) : launch_lag_reset<float>(e, mask, s); }
template <typename T>
hipError_t launch_lag_transpose(const amenv& e, void* api, int to_api, hipStream_t s) {
  const int n = e.cfg.num_envs;
  hipLaunchKernelGGL(lag_transpose_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, s, n, int(e.cfg.vehicle.n_rotors), static_cast<T*>(e.lag_w),
                     static_cast<T*>(api), to_api);
  return hipGetLastError();
}
hipError_t launch_lag_transpose(const amenv& e, void* api, int to_api, hipStream_t s) { return e.cfg.dtype == AMENV_F64 ? launch_lag_transpose<double>(e, api, to_api, s) : launch_lag_transpose<float>(e, api, to_api, s); }

// amenv_set_action_delay (off -> on) / amenv_reset: the masked envs (mask null = all; padding lanes always, as reset_kernel does) draw d for
// the episode the blob holds by now and get 8 hover rows
__global__ void delay_reset_kernel(int n, uint32_t tile_bytes, const void* __restrict__ blob, const ColdParams C, const DelayArg<true> D, const uint8_t* __restrict__ mask) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= int(D.n_pad)) return;
  if (i < n && mask && !mask[i]) return;
  const int32_t episode = iptr4(const_cast<char*>(tile_base(blob, tile_bytes, i)), i & 63)->w;
  DelayLane dl{delay_draw(C.seed_lo, C.seed_hi, D, C.gid0 + i, episode), 0};
  delay_push(D, i, dl, make_float4(1.0f, 0.0f, 0.0f, 0.0f), true);
}
// amenv_get_action_delay_state (to_api) / amenv_set_action_delay_state: d [N], rows [N][8][4] in AGE order (row k was given k + 1 steps ago)
// <-> the side buffer's ring.  The setter restarts the ring at head 0 and clamps d to 0..8.
__global__ void delay_state_kernel(int n, const DelayArg<true> D, int32_t* __restrict__ d_api, float4* __restrict__ rows_api, int to_api) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  float4* p = D.h + delay_slot(i);
  int32_t* w = delay_word(D) + i;
  if (to_api) {
    const int32_t m = *w;
    const int head = (m >> 4) & 7;
    if (d_api) d_api[i] = m & 15;
    if (rows_api)
      for (int k = 0; k < AMENV_MAX_ACTION_DELAY; k++) rows_api[size_t(i) * AMENV_MAX_ACTION_DELAY + k] = p[64 * ((head - 1 - k) & 7)];
  } else {
    const int32_t m = *w;
    int d = m & 15;
    if (d_api) d = min(max(d_api[i], 0), AMENV_MAX_ACTION_DELAY);
    if (rows_api) {
      for (int k = 0; k < AMENV_MAX_ACTION_DELAY; k++) p[64 * ((-1 - k) & 7)] = rows_api[size_t(i) * AMENV_MAX_ACTION_DELAY + k];
      *w = d;                   // head 0
    } else {
      *w = d | (m & 0x70);      // the ring stays as it is
    }
  }
}
hipError_t launch_delay_reset(const amenv& e, const uint8_t* mask, hipStream_t s) {
  hipLaunchKernelGGL(delay_reset_kernel, dim3(e.n_tiles / 4), dim3(256), 0, s, e.cfg.num_envs, e.tile_bytes, (const void*)e.blob, make_cold(e), make_delay(e), mask);
  return hipGetLastError();
}

// amenv_reset / amenv_observe while the action history is on: the task's rows (pitch od) -> the caller's (pitch od + 4 H), each ending
// in the first H rows of its env's history, most recent first (after delay_reset_kernel on the same stream: hover rows for the masked envs)
__global__ void hist_widen_kernel(int n, int od, const DelayArg<true> D, const float* __restrict__ rows, float* __restrict__ out) {
  const int w = od + 4 * D.hist;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= int64_t(n) * w) return;
  const int i = int(t / w), c = int(t % w);
  if (c < od) { out[t] = rows[size_t(i) * od + c]; return; }
  const int k = (c - od) >> 2, head = (delay_word(D)[i] >> 4) & 7;
  out[t] = reinterpret_cast<const float*>(D.h + delay_slot(i) + 64 * ((head - 1 - k) & 7))[(c - od) & 3];
}
hipError_t launch_hist_widen(const amenv& e, float* out, hipStream_t s) {
  const int64_t total = int64_t(e.cfg.num_envs) * (e.obs_dim + 4 * e.hist);
  hipLaunchKernelGGL(hist_widen_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, e.cfg.num_envs, e.obs_dim, make_delay(e), (const float*)e.hist_obs, out);
  return hipGetLastError();
}

}  // namespace

// amenv_rollout_policy[_norm] after the entry checks: pack the parameters, fill the kernel's I/O block
PolicyIO policy_io(amenv& e, const float* flat_params, uint64_t seed, uint32_t draw0, float* obs, float* actions, float* logp, float* values, float* rewards,
                   uint8_t* dones, uint32_t* info_bits, float* terminal_obs, hipStream_t s) {
  // parameters -> bf16 MFMA fragments + per-lane action constants (they change every PPO iteration): a tiny kernel in front, no host sync
  const int pack_threads = 4 * (kPolFrags + kPolBias) * 64 + 64 + 4 * 4 * 64;
  hipLaunchKernelGGL(policy_pack_kernel, dim3((pack_threads + 255) / 256), dim3(256), 0, s, flat_params, e.obs_dim + 4 * e.hist, e.act_dim, e.io_act ? e.pub_nj : 0, e.pol_pack);
  PolicyIO io;
  io.pack = reinterpret_cast<const uint4*>(e.pol_pack);
  io.seed_lo = uint32_t(seed); io.seed_hi = uint32_t(seed >> 32); io.draw0 = draw0;
  io.obs = obs; io.actions = actions; io.logp = logp; io.values = values; io.rewards = rewards; io.dones = dones; io.info = info_bits;
  io.terminal_obs = terminal_obs;
  return io;
}

namespace {
template <typename V>
__global__ void calibration_copy_kernel(const V* __restrict__ src, V* __restrict__ dst, size_t n) {
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) dst[i] = src[i];
}

}  // namespace

extern "C" {

const char* amenv_version(void) { return "amenv 0.2 (gfx950, abi 2)"; }

int amenv_default_config(const char* vehicle_name, int32_t num_envs, amenv_config* cfg) {
  if (!cfg || !vehicle_name) return fail(nullptr, AMENV_ERR_INVALID, "amenv_default_config: NULL argument");
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->struct_size = uint32_t(sizeof(*cfg));
  cfg->abi_version = AMENV_ABI_VERSION;
  cfg->num_envs = num_envs;
  cfg->dtype = AMENV_F32;
  cfg->flags = AMENV_FLAG_AUTO_RESET;
  cfg->block_size = 0;
  cfg->seed = 0;
  cfg->env_id_offset = 0;
  bool ok;
  if (!std::strcmp(vehicle_name, "quad")) ok = vehicle_quad(&cfg->vehicle);
  else if (!std::strcmp(vehicle_name, "hexa")) ok = vehicle_hexa(&cfg->vehicle);
  else if (!std::strcmp(vehicle_name, "hexa_arm")) ok = vehicle_hexa_arm(&cfg->vehicle);
  else return fail(nullptr, AMENV_ERR_INVALID, std::string("unknown vehicle '") + vehicle_name + "' (quad | hexa | hexa_arm)");
  if (!ok) return fail(nullptr, AMENV_ERR_INVALID, "singular vehicle matrices");
  fill_task_defaults(&cfg->task, 1);
  // north_star: "arm forward kinematics, waypoint reward" -- with the arm the task measures from the tool point
  cfg->task.ee_task = cfg->vehicle.n_joints > 0 ? AMENV_EE_TASK_TOOL : AMENV_EE_TASK_BASE;
  return AMENV_OK;
}

int amenv_config_set_task(amenv_config* cfg, int32_t variant) {
  if (!cfg) return AMENV_ERR_INVALID;
  if (variant == AMENV_TASK_V2_SCALED20) {
    fill_task_defaults(&cfg->task, 1);
  } else if (variant == AMENV_TASK_V1_SCALED17 || variant == AMENV_TASK_V1_RAW17) {
    fill_task_defaults(&cfg->task, 2);        // storage bound; K in {1,2} is drawn per episode (v1/rl_env_scaledObs.py:38)
    cfg->task.variant = variant;
    cfg->task.max_episode_steps = 1200;       // v1/rl_env_scaledObs.py:43
  } else {
    return fail(nullptr, AMENV_ERR_INVALID, "amenv_config_set_task: unknown variant");
  }
  return AMENV_OK;
}

int amenv_dims(const amenv_config* cfg, int32_t* obs_dim, int32_t* act_dim, int32_t* nff, int32_t* nif) {
  if (!cfg) return AMENV_ERR_INVALID;
  if (obs_dim) *obs_dim = obs_dim_of(cfg);
  if (act_dim) *act_dim = act_dim_of(cfg);
  if (nff) *nff = n_float_fields(cfg);
  if (nif) *nif = AMENV_I_NFIELDS;
  return AMENV_OK;
}

// DESIGN.md "Algorithmic bytes": what one env-step of amenv_step() must move through HBM.
int64_t amenv_bytes_per_env_step(const amenv_config* cfg) {
  if (!cfg) return 0;
  const int64_t ts = cfg->dtype == AMENV_F64 ? 8 : 4;
  const int64_t K = cfg->task.num_waypoints;
  const int64_t nj = cfg->vehicle.n_joints;
  const int64_t rd = ts * (13 /*state*/ + 1 /*final_yaw*/ + 1 /*last_distance*/ + 1 /*ep_return*/ + 3 * K /*waypoints*/ + 2 * nj /*joints*/) +
                     4 * 3 /*step,counter,flags*/ + 4 * act_dim_of(cfg) /*action*/;
  const int64_t wr = ts * (13 + 1 + 1 + 2 * nj) + 4 * 3 + 4 * obs_dim_of(cfg) /*obs*/ + ts /*reward*/ + 1 /*done*/ + 4 /*info*/;
  return rd + wr;
}

// ---- n-link arm, n < 3: boundary adapters (see struct amenv) ---------------------------------------------------------------------
namespace {
__global__ void arm_pad_actions_kernel(const float* __restrict__ a, int n, int nj, float* __restrict__ out) {   // [N][4 + nj] -> [N][7]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 7) return;
  const int e = i / 7, k = i % 7;
  out[i] = k < 4 + nj ? a[e * (4 + nj) + k] : 0.0f;
}
// internal rows [N][29] = 20 | th(3) | thd(3) | tool(3)  ->  public rows [N][20 + 2 nj + 3]; rows_of: only rows with a non-zero byte (terminal rows)
__global__ void arm_cut_obs_kernel(const float* __restrict__ in, int n, int nj, const uint8_t* __restrict__ rows_of, float* __restrict__ out) {
  const int od = 23 + 2 * nj;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * od) return;
  const int e = i / od, k = i % od;
  if (rows_of && !rows_of[e]) return;
  const int src = k < 20 ? k : (k < 20 + nj ? k : (k < 20 + 2 * nj ? 23 + (k - 20 - nj) : 26 + (k - 20 - 2 * nj)));
  out[i] = in[e * 29 + src];
}
// the 3-joint vehicle with phantom links behind the caller's n (1 or 2) real ones
amenv_config pad_arm_config(const amenv_config& c) {
  amenv_config p = c;
  amenv_vehicle& v = p.vehicle;
  for (int k = c.vehicle.n_joints; k < 3; k++) {
    v.link_mass[k] = 0.0;
    for (int j = 0; j < 3; j++) { v.joint_origin[3 * k + j] = 0.0; v.link_com[3 * k + j] = 0.0; v.joint_axis[3 * k + j] = j == 0 ? 1.0 : 0.0; }   // x axis: keeps a z[,x] arm on the z,x,x kernels
    for (int j = 0; j < 9; j++) v.link_inertia[9 * k + j] = 0.0;
    v.joint_limit[2 * k] = v.joint_limit[2 * k + 1] = 0.0;
  }
  v.n_joints = 3;
  return p;
}
}  // namespace

int amenv_create(const amenv_config* cfg, int device, amenv** out) {
  if (!out) return fail(nullptr, AMENV_ERR_INVALID, "amenv_create: out is NULL");
  *out = nullptr;
  if (const char* why = validate(cfg)) return fail(nullptr, AMENV_ERR_INVALID, std::string("amenv_create: ") + why);
  const amenv_config user_cfg = *cfg;                       // the caller's dimensions (obs / action / state fields)
  const int pub_nj = user_cfg.vehicle.n_joints;
  const amenv_config icfg = (pub_nj == 1 || pub_nj == 2) ? pad_arm_config(user_cfg) : user_cfg;   // the (internal) vehicle the kernels run
  StepFamily family;
  if (const char* why = select_step_family(icfg, &family)) return fail(nullptr, AMENV_ERR_INVALID, std::string("amenv_create: ") + why);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, AMENV_ERR_NO_DEVICE, "amenv_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(nullptr, AMENV_ERR_INVALID, "amenv_create: device index out of range");
  hipDeviceProp_t prop;
  AMENV_HIP(nullptr, hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, AMENV_ERR_NO_DEVICE, std::string("amenv_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  amenv* e = new (std::nothrow) amenv();
  if (!e) return fail(nullptr, AMENV_ERR_ALLOC, "amenv_create: out of host memory");
  e->pub_nj = pub_nj;
  e->cfg = icfg;
  e->family = family;
  cfg = &e->cfg;                                            // everything below sets up the (internal) vehicle the kernels run
  e->device = device;
  e->nf = n_float_fields(&user_cfg);
  const size_t n = size_t(cfg->num_envs), ts = cfg->dtype == AMENV_F64 ? 8 : 4;
  e->fbytes = size_t(e->nf) * n * ts;
  e->ibytes = size_t(AMENV_I_NFIELDS) * n * sizeof(int32_t);
  // tiles are allocated in multiples of 4 (= 256 lanes, the largest workgroup): every launch geometry stays inside the blob and
  // every padding lane holds a valid environment (initialised below), so kernels never need a per-lane bounds branch on the state
  e->n_tiles = int((n + 255) / 256) * 4;
  e->tile_bytes = tile_bytes_for(cfg->task.num_waypoints, cfg->vehicle.n_joints, int(ts));
  e->blob_bytes = size_t(e->n_tiles) * e->tile_bytes;
  // latency regime (few waves per CU): one wave per workgroup spreads the waves over more CUs;
  // throughput regime: 256-thread workgroups
  e->block = cfg->block_size ? cfg->block_size : (cfg->num_envs <= 65536 ? 64 : 256);
  e->obs_dim = obs_dim_of(&user_cfg);
  e->act_dim = act_dim_of(&user_cfg);
  e->kname = kernel_name(*e);
  auto alloc_failed = [e](const char* what, hipError_t s) {
    const std::string msg = std::string("amenv_create: ") + what + ": " + hipGetErrorString(s);
    amenv_destroy(e);
    return fail(nullptr, AMENV_ERR_ALLOC, msg);
  };
  DeviceGuard g(device);
  hipError_t s;
  if ((s = hipMalloc(&e->blob, e->blob_bytes)) != hipSuccess ||
      (s = hipMalloc((void**)&e->stats, sizeof(unsigned long long) * kStatsWords)) != hipSuccess ||
      (s = hipMemset(e->blob, 0, e->blob_bytes)) != hipSuccess ||
      (s = hipMemset(e->stats, 0, sizeof(unsigned long long) * kStatsWords)) != hipSuccess ||
      // give the padding lanes of the last tile a valid state (real envs stay untouched: episode 0)
      (s = launch_reset(*e, nullptr, nullptr, 1, nullptr)) != hipSuccess ||
      (s = hipDeviceSynchronize()) != hipSuccess)
    return alloc_failed("device allocation failed", s);
  // the lane-quad / fp32 lane-team constants (every kernel of theirs: step, rollout, closed-loop rollout) + the packed policy of amenv_rollout_policy
  const bool quad = quad_ok(*cfg), team = team_ok(*cfg);
  if (rigid_pol_ok(*cfg) || arm_pol_ok(*cfg))   // (quad_ok implies rigid_pol_ok, team_ok arm_pol_ok)
    if ((s = hipMalloc((void**)&e->pol_pack, size_t(kPolPackWords) * sizeof(uint32_t))) != hipSuccess) return alloc_failed("policy pack", s);
  if ((quad || team) && (s = upload_team_consts<float>(e, team)) != hipSuccess) return alloc_failed(quad ? "quad constants" : "team constants", s);
  if (family == StepFamily::Team && cfg->dtype == AMENV_F64 && (s = upload_team_consts<double>(e, true)) != hipSuccess) return alloc_failed("team constants (fp64)", s);
  if (e->pub_nj == 1 || e->pub_nj == 2) {
    if ((s = hipMalloc((void**)&e->io_act, n * 7 * sizeof(float))) != hipSuccess || (s = hipMalloc((void**)&e->io_obs, n * 29 * sizeof(float))) != hipSuccess ||
        (s = hipMalloc((void**)&e->io_term, n * 29 * sizeof(float))) != hipSuccess)
      return alloc_failed("n-link adapter buffers", s);
  }
  *out = e;
  return AMENV_OK;
}

int amenv_destroy(amenv* e) {
  if (!e) return AMENV_OK;
  {
    DeviceGuard g(e->device);
    if (e->blob) (void)hipFree(e->blob);
    if (e->stats) (void)hipFree(e->stats);
    if (e->team_consts) (void)hipFree(e->team_consts);
    if (e->pol_pack) (void)hipFree(e->pol_pack);
    if (e->lag_w) (void)hipFree(e->lag_w);
    if (e->delay_h) (void)hipFree(e->delay_h);
    if (e->hist_obs) (void)hipFree(e->hist_obs);
    if (e->io_act) (void)hipFree(e->io_act);
    if (e->io_obs) (void)hipFree(e->io_obs);
    if (e->io_term) (void)hipFree(e->io_term);
    if (e->ev_start) (void)hipEventDestroy(e->ev_start);
    if (e->ev_stop) (void)hipEventDestroy(e->ev_stop);
  }
  delete e;
  return AMENV_OK;
}

const char* amenv_last_error(const amenv* e) { return e ? e->err.c_str() : g_create_err.c_str(); }
const char* amenv_kernel_name(const amenv* e) { return e ? (e->kname = kernel_name(*e)).c_str() : ""; }   // of the handle's state by now: no setter keeps it current

}  // extern "C"

hipError_t pad_actions(const amenv& e, const float* actions, hipStream_t s) {
  const int n = e.cfg.num_envs;
  hipLaunchKernelGGL(arm_pad_actions_kernel, dim3((n * 7 + 255) / 256), dim3(256), 0, s, actions, n, e.pub_nj, e.io_act);
  return hipGetLastError();
}
hipError_t cut_obs(const amenv& e, const float* rows29, const uint8_t* rows_of, float* out, hipStream_t s) {
  const int n = e.cfg.num_envs, od = 23 + 2 * e.pub_nj;
  hipLaunchKernelGGL(arm_cut_obs_kernel, dim3((n * od + 255) / 256), dim3(256), 0, s, rows29, n, e.pub_nj, rows_of, out);
  return hipGetLastError();
}

extern "C" {

int amenv_set_seed(amenv* e, uint64_t seed) {
  if (!e) return AMENV_ERR_INVALID;
  e->cfg.seed = seed;
  return AMENV_OK;
}

namespace {
// What the rigid kernels' opt-in switches serve, checked by every setter (who, for the messages): rigid vehicles with 4 or 6 rotors off the lane-quad
// family, fp32 handles where the switch's kernels are fp32 only.  AMENV_OK, or the failure already recorded in the handle.  (pub_nj > 0 implies
// cfg.vehicle.n_joints == 3, so the clause the delay's check had changes nothing for the setters that tested n_joints alone.)
int rigid_switch_served(amenv* e, const std::string& who, bool needs_f32, const char* arm_reason = "the arm kernels are not built with it") {
  const int nr = e->cfg.vehicle.n_rotors;
  if (e->cfg.vehicle.n_joints > 0 || e->pub_nj > 0) return fail(e, AMENV_ERR_INVALID, who + ": built for rigid vehicles (" + arm_reason + ")");
  if (nr != 4 && nr != 6) return fail(e, AMENV_ERR_INVALID, who + ": built for rigid vehicles with 4 or 6 rotors");
  if (needs_f32 && e->cfg.dtype != AMENV_F32) return fail(e, AMENV_ERR_INVALID, who + ": fp32 handles only (the fp64 builds are logic gates of the dynamics)");
  if (e->family == StepFamily::Quad)
    return fail(e, AMENV_ERR_INVALID, who + ": the lane-quad step kernel (step_kernel = AMENV_KERNEL_TEAM on a rigid vehicle) is not built with it; "
                "use the lane or helper kernel");
  return AMENV_OK;
}
}  // namespace

int amenv_set_randomization(amenv* e, const amenv_randomization* r) {
  if (!e) return AMENV_ERR_INVALID;
  if (!r) {
    e->dr = false;
    e->dr_r = DrRanges{{1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f}};
    return AMENV_OK;
  }
  if (r->struct_size != sizeof(amenv_randomization)) return fail(e, AMENV_ERR_INVALID, "amenv_set_randomization: struct_size must be sizeof(amenv_randomization)");
  if (int rc = rigid_switch_served(e, "amenv_set_randomization", false, "an arm vehicle's mass and inertia are not one scalar scale")) return rc;
  const float* rg[3] = {r->mass_scale, r->inertia_scale, r->thrust_scale};
  const char* nm[3] = {"mass_scale", "inertia_scale", "thrust_scale"};
  for (int q = 0; q < 3; q++) {
    const float lo = rg[q][0], hi = rg[q][1];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo >= 0.25f) || !(lo <= hi) || !(hi <= 4.0f))
      return fail(e, AMENV_ERR_INVALID, std::string("amenv_set_randomization: ") + nm[q] + " must be finite with 0.25 <= lo <= hi <= 4");
  }
  DrRanges R;
  for (int q = 0; q < 3; q++) { R.lo[q] = rg[q][0]; R.span[q] = rg[q][1] - rg[q][0]; }
  e->dr = true;
  e->dr_r = R;
  return AMENV_OK;
}

int amenv_dynamics_factors(amenv* e, float* out, void* stream) {
  if (!e || !out) return fail(e, AMENV_ERR_INVALID, "amenv_dynamics_factors: NULL argument");
  const int nr = e->cfg.vehicle.n_rotors, n = e->cfg.num_envs;
  if (e->cfg.vehicle.n_joints > 0 || (nr != 4 && nr != 6))
    return fail(e, AMENV_ERR_INVALID, "amenv_dynamics_factors: built for rigid vehicles with 4 or 6 rotors");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((n + 255) / 256), block(256);
  with_rotors46(nr, [&](auto nrot) { hipLaunchKernelGGL(dr_factors_kernel<decltype(nrot)::value>, grid, block, 0, s, n, e->tile_bytes, (const void*)e->blob, make_cold(*e), e->dr_r, out); });
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

int amenv_set_sensor_noise(amenv* e, const amenv_sensor_noise* z) {
  if (!e) return AMENV_ERR_INVALID;
  const NoiseSig off = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!z) {   // off: the handle launches the kernels it launched before
    e->noise = false; e->noise_s = off;
    return AMENV_OK;
  }
  if (z->struct_size != sizeof(amenv_sensor_noise)) return fail(e, AMENV_ERR_INVALID, "amenv_set_sensor_noise: struct_size must be sizeof(amenv_sensor_noise)");
  const float sg[4] = {z->sigma_position, z->sigma_velocity, z->sigma_rate, z->sigma_attitude};
  const char* nm[4] = {"sigma_position", "sigma_velocity", "sigma_rate", "sigma_attitude"};
  for (int q = 0; q < 4; q++)
    if (!std::isfinite(sg[q]) || !(sg[q] >= 0.0f) || !(sg[q] <= 1.0f))
      return fail(e, AMENV_ERR_INVALID, std::string("amenv_set_sensor_noise: ") + nm[q] + " must be finite with 0 <= sigma <= 1");
  if (int rc = rigid_switch_served(e, "amenv_set_sensor_noise", true)) return rc;
  if (e->cfg.task.max_episode_steps > (1 << 22) - 2)
    return fail(e, AMENV_ERR_INVALID, "amenv_set_sensor_noise: max_episode_steps must be <= 2^22 - 2 (the step field of the draw's counter has 22 bits)");
  const bool any = sg[0] != 0.0f || sg[1] != 0.0f || sg[2] != 0.0f || sg[3] != 0.0f;   // all zeros: the same as off
  e->noise = any;
  e->noise_s = any ? NoiseSig{sg[0], sg[1], sg[2], sg[3]} : off;
  return AMENV_OK;
}

int amenv_sensor_noise_samples(amenv* e, float* out, void* stream) {
  if (!e || !out) return fail(e, AMENV_ERR_INVALID, "amenv_sensor_noise_samples: NULL argument");
  const int nr = e->cfg.vehicle.n_rotors, n = e->cfg.num_envs;
  if (e->cfg.vehicle.n_joints > 0 || (nr != 4 && nr != 6) || e->cfg.dtype != AMENV_F32)
    return fail(e, AMENV_ERR_INVALID, "amenv_sensor_noise_samples: built for fp32 rigid vehicles with 4 or 6 rotors");
  DeviceGuard g(e->device);
  hipLaunchKernelGGL(noise_samples_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, e->tile_bytes, (const void*)e->blob, make_cold(*e), out);
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

int amenv_set_rotor_lag(amenv* e, const amenv_rotor_lag* lag) {
  if (!e) return AMENV_ERR_INVALID;
  if (!lag) {   // off: the handle launches the kernels it launched before (the side buffer stays allocated, unused)
    e->lag = false;
    return AMENV_OK;
  }
  const amenv_vehicle& v = e->cfg.vehicle;
  if (lag->struct_size != sizeof(amenv_rotor_lag)) return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_lag: struct_size must be sizeof(amenv_rotor_lag)");
  if (int rc = rigid_switch_served(e, "amenv_set_rotor_lag", false)) return rc;
  for (int r = 0; r < v.n_rotors; r++)
    if (!(v.t_min[r] >= 0.0)) return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_lag: every t_min must be >= 0 (the rotor state is the square root of a thrust)");
  const double tau[2] = {lag->tau_up, lag->tau_down};
  for (int q = 0; q < 2; q++)
    if (!std::isfinite(tau[q]) || !(tau[q] > 0.0) || !(tau[q] <= 10.0))
      return fail(e, AMENV_ERR_INVALID, std::string("amenv_set_rotor_lag: ") + (q ? "tau_down" : "tau_up") + " must be finite with 0 < tau <= 10 (seconds)");
  DeviceGuard g(e->device);
  if (!e->lag_w) {   // first enable: the one allocation, and w0 (a function of the config alone) behind the states
    const bool f64 = e->cfg.dtype == AMENV_F64;
    const size_t ts = f64 ? 8 : 4, states = size_t(v.n_rotors) * size_t(e->n_tiles) * 64;
    double w0d[AMENV_MAX_ROTORS]; float w0f[AMENV_MAX_ROTORS];
    for (int r = 0; r < v.n_rotors; r++) { w0d[r] = lag_w0(v, r); w0f[r] = float(w0d[r]); }
    void* buf = nullptr;
    hipError_t st = hipMalloc(&buf, (states + size_t(v.n_rotors)) * ts);
    if (st != hipSuccess) return fail(e, AMENV_ERR_ALLOC, std::string("amenv_set_rotor_lag: hipMalloc: ") + hipGetErrorString(st));
    st = hipMemcpy(static_cast<char*>(buf) + states * ts, f64 ? static_cast<const void*>(w0d) : static_cast<const void*>(w0f), size_t(v.n_rotors) * ts, hipMemcpyHostToDevice);
    if (st != hipSuccess) { (void)hipFree(buf); return fail(e, AMENV_ERR_HIP, std::string("amenv_set_rotor_lag: hipMemcpy: ") + hipGetErrorString(st)); }
    e->lag_w = buf;
  }
  const bool was_on = e->lag;
  for (int q = 0; q < 2; q++) e->lag_a[q] = -std::expm1(-e->cfg.task.dt / tau[q]);
  e->lag = true;
  if (!was_on) {     // off -> on: every rotor at the nominal hover command; on -> on keeps the states (curricula)
    AMENV_HIP(e, launch_lag_reset(*e, nullptr, nullptr));
    AMENV_HIP(e, hipDeviceSynchronize());
  }
  return AMENV_OK;
}

namespace {
// The side buffer of amenv_set_action_delay and amenv_set_action_history (one: the history IS the delay's buffer): its one allocation.
int delay_buffer(amenv* e, const std::string& who) {   // (under a DeviceGuard)
  if (e->delay_h) return AMENV_OK;
  const size_t n_pad = size_t(e->n_tiles) * 64;
  void* buf = nullptr;
  hipError_t st = hipMalloc(&buf, n_pad * (AMENV_MAX_ACTION_DELAY * sizeof(float4) + sizeof(int32_t)));
  if (st != hipSuccess) return fail(e, AMENV_ERR_ALLOC, who + ": hipMalloc: " + hipGetErrorString(st));
  e->delay_h = buf;
  return AMENV_OK;
}
}  // namespace

int amenv_set_action_delay(amenv* e, const amenv_action_delay* z) {
  if (!e) return AMENV_ERR_INVALID;
  if (!z) {   // off: the handle launches the kernels it launched before (the side buffer stays allocated, unused) -- or, while the action history is
    // on, the DELAY kernels with range (0, 0): every env keeps its d and its rows, the episodes that start from now on draw 0
    e->delay = false;
    return AMENV_OK;
  }
  if (z->struct_size != sizeof(amenv_action_delay)) return fail(e, AMENV_ERR_INVALID, "amenv_set_action_delay: struct_size must be sizeof(amenv_action_delay)");
  if (z->min_steps < 0 || z->min_steps > z->max_steps || z->max_steps > AMENV_MAX_ACTION_DELAY)
    return fail(e, AMENV_ERR_INVALID, "amenv_set_action_delay: need 0 <= min_steps <= max_steps <= AMENV_MAX_ACTION_DELAY (8)");
  if (int rc = rigid_switch_served(e, "amenv_set_action_delay", true)) return rc;
  DeviceGuard g(e->device);
  if (int rc = delay_buffer(e, "amenv_set_action_delay")) return rc;   // first enable: the one allocation
  const bool was_on = e->delay;
  e->delay_lo = z->min_steps; e->delay_hi = z->max_steps;
  e->delay = true;
  if (!was_on) {     // off -> on: every env draws d for its current episode and gets hover rows; on -> on keeps d and the rows (curricula)
    AMENV_HIP(e, launch_delay_reset(*e, nullptr, nullptr));
    AMENV_HIP(e, hipDeviceSynchronize());
  }
  return AMENV_OK;
}

int amenv_set_action_history(amenv* e, int32_t rows) {
  if (!e) return AMENV_ERR_INVALID;
  if (rows < 0 || rows > 2) return fail(e, AMENV_ERR_INVALID, "amenv_set_action_history: rows must be 0 (off), 1 or 2");
  if (rows == 0) {   // off: base-width rows again; without the delay the handle launches the kernels it launched before (the buffers stay allocated, unused)
    e->hist = 0;
    return AMENV_OK;
  }
  if (int rc = rigid_switch_served(e, "amenv_set_action_history", true)) return rc;
  DeviceGuard g(e->device);
  if (int rc = delay_buffer(e, "amenv_set_action_history")) return rc;   // the delay's side buffer IS the history
  if (!e->hist_obs) {
    void* buf = nullptr;
    hipError_t st = hipMalloc(&buf, size_t(e->cfg.num_envs) * e->obs_dim * sizeof(float));
    if (st != hipSuccess) return fail(e, AMENV_ERR_ALLOC, std::string("amenv_set_action_history: hipMalloc: ") + hipGetErrorString(st));
    e->hist_obs = static_cast<float*>(buf);
  }
  const bool buffer_live = e->delay_path();   // the delay or the history has kept the buffer current
  e->hist = rows;
  if (!buffer_live) {   // neither was on: hover rows, and d = 0 from the range (0, 0)
    AMENV_HIP(e, launch_delay_reset(*e, nullptr, nullptr));
    AMENV_HIP(e, hipDeviceSynchronize());
  }
  return AMENV_OK;
}

int32_t amenv_obs_dim(const amenv* e) { return e ? e->obs_dim + 4 * e->hist : 0; }

int amenv_set_rate_control(amenv* e, const amenv_rate_control* r) {
  if (!e) return AMENV_ERR_INVALID;
  if (!r) {   // off: the handle launches the kernels it launched before
    e->rate = RateBlock{0, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
    return AMENV_OK;
  }
  if (int rc = rigid_switch_served(e, "amenv_set_rate_control", true)) return rc;
  const char* ax[3] = {"x", "y", "z"};
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(r->max_rate[k]) || !(r->max_rate[k] > 0.0) || !std::isfinite(float(r->max_rate[k])))
      return fail(e, AMENV_ERR_INVALID, std::string("amenv_set_rate_control: max_rate ") + ax[k] + " must be finite and > 0 (rad/s)");
    if (!std::isfinite(r->gain[k]) || !(r->gain[k] > 0.0) || !(float(r->gain[k]) > 0.0f))
      return fail(e, AMENV_ERR_INVALID, std::string("amenv_set_rate_control: gain ") + ax[k] + " must be finite and > 0 (1/s)");
    if (!(r->gain[k] * e->cfg.task.dt < 1.0))
      return fail(e, AMENV_ERR_INVALID, std::string("amenv_set_rate_control: gain ") + ax[k] + " * task.dt must be < 1 (past that the held torque overshoots the command within one step)");
  }
  RateBlock Q;
  Q.on = r->gyro_feedforward ? 3 : 1;
  for (int k = 0; k < 3; k++) { Q.max_rate[k] = float(r->max_rate[k]); Q.gain[k] = float(r->gain[k]); }
  Q.inv_ms = float(1.0 / double(float(e->cfg.vehicle.moment_scale)));   // of the fp32 scale the step multiplies a' by (HotParams::mscale_f)
  if (!std::isfinite(Q.inv_ms) || Q.inv_ms == 0.0f) return fail(e, AMENV_ERR_INVALID, "amenv_set_rate_control: the vehicle's moment_scale has no finite fp32 reciprocal");
  e->rate = Q;
  return AMENV_OK;
}

int amenv_rate_moment_actions(amenv* e, const float* actions, float* out, void* stream) {
  if (!e || !actions || !out) return fail(e, AMENV_ERR_INVALID, "amenv_rate_moment_actions: NULL argument");
  if (!e->rate.on) return fail(e, AMENV_ERR_INVALID, "amenv_rate_moment_actions: rate control is off (amenv_set_rate_control)");
  if (!aligned16(actions) || !aligned16(out)) return fail(e, AMENV_ERR_INVALID, "amenv_rate_moment_actions: actions / out must be 16-byte aligned");
  DeviceGuard g(e->device);
  const int n = e->cfg.num_envs;
  with_rotors46(e->cfg.vehicle.n_rotors, [&](auto nrot) {
    constexpr int NROT = decltype(nrot)::value;
    hipLaunchKernelGGL(rate_moment_kernel<NROT>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, e->tile_bytes, (const void*)e->blob, make_hot<float, NROT>(*e), e->rate,
                       reinterpret_cast<const float4*>(actions), reinterpret_cast<float4*>(out));
  });
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

int amenv_set_rotor_failure(amenv* e, const amenv_rotor_failure* f) {
  if (!e) return AMENV_ERR_INVALID;
  if (!f) {   // off: the handle launches the kernels it launched before
    e->fail = FailBlock{0u, 0u, 0u, 0.0f, 0.0f};
    return AMENV_OK;
  }
  if (f->struct_size != sizeof(amenv_rotor_failure)) return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_failure: struct_size must be sizeof(amenv_rotor_failure)");
  if (int rc = rigid_switch_served(e, "amenv_set_rotor_failure", false)) return rc;   // (fp64 too, as randomisation: the oracle gate runs there)
  const int nr = e->cfg.vehicle.n_rotors;
  if (!std::isfinite(f->probability) || !(f->probability >= 0.0f) || !(f->probability <= 1.0f))
    return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_failure: probability must be finite, 0..1");
  if (f->onset_min < 0 || f->onset_min > f->onset_max || f->onset_max > 65535)
    return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_failure: onset must be a range of control steps with 0 <= min <= max <= 65535");
  if (!std::isfinite(f->remaining_min) || !std::isfinite(f->remaining_max) || !(f->remaining_min >= 0.0f) || !(f->remaining_min <= f->remaining_max) || !(f->remaining_max <= 1.0f))
    return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_failure: remaining must be finite with 0 <= min <= max <= 1");
  const uint32_t all = (1u << nr) - 1u;
  if (f->rotor_mask & ~all) return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_failure: rotor_mask has a bit at or above the vehicle's rotor count");
  const uint32_t p16 = uint32_t(std::floor(double(f->probability) * 65536.0 + 0.5));   // 0: never, 65536: always (the draw's half is below 65536)
  const uint32_t mask = f->rotor_mask ? f->rotor_mask : all;
  FailBlock X;
  X.ctl = 0x80000000u | uint32_t(__builtin_popcount(mask)) << 17 | p16;
  X.rotors = 0u;
  for (int r = 0, k = 0; r < nr; r++)
    if ((mask >> r) & 1u) X.rotors |= uint32_t(r) << (4 * k++);   // the admissible rotors in ascending order
  X.onset = uint32_t(f->onset_min) | uint32_t(f->onset_max - f->onset_min) << 16;
  X.rem_lo = f->remaining_min; X.rem_span = f->remaining_max - f->remaining_min;
  e->fail = X;
  return AMENV_OK;
}

int amenv_rotor_failure_state(amenv* e, int32_t* plan, float* factors, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!plan && !factors) return fail(e, AMENV_ERR_INVALID, "amenv_rotor_failure_state: NULL arguments");
  if (!e->fail.ctl) return fail(e, AMENV_ERR_INVALID, "amenv_rotor_failure_state: the rotor failure is off (amenv_set_rotor_failure)");
  DeviceGuard g(e->device);
  const int n = e->cfg.num_envs;
  with_rotors46(e->cfg.vehicle.n_rotors, [&](auto nrot) {
    hipLaunchKernelGGL(fail_state_kernel<decltype(nrot)::value>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, e->tile_bytes, (const void*)e->blob, make_cold(*e), e->fail,
                       plan, factors);
  });
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

int amenv_get_action_delay_state(amenv* e, int32_t* d_out, float* recent_out, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!d_out && !recent_out) return fail(e, AMENV_ERR_INVALID, "amenv_get_action_delay_state: NULL arguments");
  if (!e->delay_path()) return fail(e, AMENV_ERR_INVALID, "amenv_get_action_delay_state: the action delay and the action history are off (amenv_set_action_delay, amenv_set_action_history)");
  if (recent_out && !aligned16(recent_out)) return fail(e, AMENV_ERR_INVALID, "amenv_get_action_delay_state: recent_out must be 16-byte aligned");
  DeviceGuard g(e->device);
  const int n = e->cfg.num_envs;
  hipLaunchKernelGGL(delay_state_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, make_delay(*e), d_out, reinterpret_cast<float4*>(recent_out), 1);
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

int amenv_set_action_delay_state(amenv* e, const int32_t* d_in, const float* recent_in, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!d_in && !recent_in) return fail(e, AMENV_ERR_INVALID, "amenv_set_action_delay_state: NULL arguments");
  if (!e->delay_path()) return fail(e, AMENV_ERR_INVALID, "amenv_set_action_delay_state: the action delay and the action history are off (amenv_set_action_delay, amenv_set_action_history)");
  if (recent_in && !aligned16(recent_in)) return fail(e, AMENV_ERR_INVALID, "amenv_set_action_delay_state: recent_in must be 16-byte aligned");
  DeviceGuard g(e->device);
  const int n = e->cfg.num_envs;
  hipLaunchKernelGGL(delay_state_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, make_delay(*e), const_cast<int32_t*>(d_in),
                     reinterpret_cast<float4*>(const_cast<float*>(recent_in)), 0);
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

int amenv_get_rotor_state(amenv* e, void* out, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!out) return fail(e, AMENV_ERR_INVALID, "amenv_get_rotor_state: NULL argument");
  if (!e->lag) return fail(e, AMENV_ERR_INVALID, "amenv_get_rotor_state: the rotor lag is off (amenv_set_rotor_lag)");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  AMENV_HIP(e, launch_lag_transpose(*e, out, 1, s));
  return AMENV_OK;
}

int amenv_set_rotor_state(amenv* e, const void* in, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!in) return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_state: NULL argument");
  if (!e->lag) return fail(e, AMENV_ERR_INVALID, "amenv_set_rotor_state: the rotor lag is off (amenv_set_rotor_lag)");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  AMENV_HIP(e, launch_lag_transpose(*e, const_cast<void*>(in), 0, s));
  return AMENV_OK;
}

int amenv_reset(amenv* e, const uint8_t* mask, float* obs_out, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  float* o = (e->io_obs && obs_out) ? e->io_obs : (e->hist && obs_out) ? e->hist_obs : obs_out;   // (the history is refused on the arms: at most one of the two)
  AMENV_HIP(e, launch_reset(*e, mask, o, 0, s));
  if (e->lag) AMENV_HIP(e, launch_lag_reset(*e, mask, s));
  if (e->delay_path()) AMENV_HIP(e, launch_delay_reset(*e, mask, s));
  if (o == e->hist_obs && o) AMENV_HIP(e, launch_hist_widen(*e, obs_out, s));   // hover rows for the masked envs, the current history for the others
  else if (o != obs_out) AMENV_HIP(e, cut_obs(*e, e->io_obs, nullptr, obs_out, s));
  return AMENV_OK;
}

int amenv_observe(amenv* e, float* obs_out, void* stream) {
  if (!e || !obs_out) return fail(e, AMENV_ERR_INVALID, "amenv_observe: NULL argument");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  float* o = e->io_obs ? e->io_obs : e->hist ? e->hist_obs : obs_out;
  AMENV_HIP(e, launch_observe(*e, o, nullptr, s));
  if (e->hist) AMENV_HIP(e, launch_hist_widen(*e, obs_out, s));
  else if (o != obs_out) AMENV_HIP(e, cut_obs(*e, e->io_obs, nullptr, obs_out, s));
  return AMENV_OK;
}

int amenv_ee_position(amenv* e, float* ee_out, void* stream) {
  if (!e || !ee_out) return fail(e, AMENV_ERR_INVALID, "amenv_ee_position: NULL argument");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  AMENV_HIP(e, launch_observe(*e, nullptr, ee_out, s));
  return AMENV_OK;
}

int amenv_get_state(amenv* e, void* fstate, int32_t* istate, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  AMENV_HIP(e, launch_transpose(*e, fstate, istate, 1, s));
  return AMENV_OK;
}

int amenv_set_state(amenv* e, const void* fstate, const int32_t* istate, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  AMENV_HIP(e, launch_transpose(*e, const_cast<void*>(fstate), const_cast<int32_t*>(istate), 0, s));
  return AMENV_OK;
}

int amenv_stats_read(amenv* e, amenv_stats* out, int reset, void* stream) {
  if (!e || !out) return fail(e, AMENV_ERR_INVALID, "amenv_stats_read: NULL argument");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  // the totals live in kStatsReplicas copies (contention-free atomics, amenv_kernels.hpp): one copy of all of them, summed here
  static_assert(S_COUNT <= kStatsStride, "stats replica stride");
  std::vector<unsigned long long> rep(size_t(kStatsReplicas) * kStatsStride);
  AMENV_HIP(e, hipMemcpyAsync(rep.data(), e->stats, rep.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (reset) AMENV_HIP(e, hipMemsetAsync(e->stats, 0, rep.size() * sizeof(unsigned long long), s));
  AMENV_HIP(e, hipStreamSynchronize(s));
  unsigned long long h[S_COUNT] = {0};
  for (int r = 0; r < kStatsReplicas; r++)
    for (int k = 0; k < S_COUNT; k++) h[k] += rep[size_t(r) * kStatsStride + k];
  out->steps = e->steps;
  out->episodes = h[S_EPISODES]; out->terminated = h[S_TERMINATED]; out->truncated = h[S_TRUNCATED];
  out->success = h[S_SUCCESS]; out->crashed = h[S_CRASHED]; out->oob = h[S_OOB]; out->nonfinite = h[S_NONFINITE];
  out->length_sum = h[S_LENGTH]; out->return_sum_q10 = (int64_t)h[S_RETURN_Q10];
  if (reset) e->steps = 0;
  return AMENV_OK;
}

// ---- observation normaliser ------------------------------------------------------------------------------------------
int amenv_obsnorm_create(int32_t dim, int device, amenv_obsnorm** out) {
  if (!out || dim <= 0 || dim > 1024) return fail(nullptr, AMENV_ERR_INVALID, "amenv_obsnorm_create: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(nullptr, AMENV_ERR_NO_DEVICE, "amenv_obsnorm_create: no such HIP device");
  amenv_obsnorm* h = new (std::nothrow) amenv_obsnorm();
  if (!h) return AMENV_ERR_ALLOC;
  h->dim = dim; h->device = device;
  DeviceGuard g(device);
  if (hipMalloc((void**)&h->buf, sizeof(double) * obsnorm_words(dim)) != hipSuccess) { delete h; return fail(nullptr, AMENV_ERR_ALLOC, "amenv_obsnorm_create: hipMalloc failed"); }
  std::string zero_one(sizeof(double) * obsnorm_words(dim), '\0');
  double* init = reinterpret_cast<double*>(&zero_one[0]);
  for (int j = 0; j < dim; j++) init[dim + j] = 1.0;   // var = 1
  init[2 * dim] = 1e-4;                                 // count = epsilon (sb3 RunningMeanStd default)
  if (hipMemcpy(h->buf, init, zero_one.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(h->buf); delete h; return fail(nullptr, AMENV_ERR_HIP, "amenv_obsnorm_create: init copy failed"); }
  *out = h;
  return AMENV_OK;
}

int amenv_obsnorm_destroy(amenv_obsnorm* h) {
  if (!h) return AMENV_OK;
  { DeviceGuard g(h->device); if (h->buf) (void)hipFree(h->buf); }
  delete h;
  return AMENV_OK;
}

int amenv_obsnorm_update(amenv_obsnorm* h, const float* obs, int64_t n, void* stream) {
  if (!h || !obs || n <= 0) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int d = h->dim, bs = 256;
  const long long n_elems = (long long)n * d;
  long long blocks = (n_elems + bs - 1) / bs;
  if (blocks > 1024) blocks = 1024;
  long long stride = blocks * bs;
  stride = ((stride + d - 1) / d) * d;             // multiple of d: a thread stays on one column
  blocks = (stride + bs - 1) / bs;
  hipLaunchKernelGGL(obsnorm_sum_kernel, dim3((unsigned)blocks), dim3(bs), sizeof(double) * 2 * d, s, obs, n_elems, d, stride, h->buf);
  hipLaunchKernelGGL(obsnorm_merge_kernel, dim3(1), dim3(((d + 63) / 64) * 64), 0, s, h->buf, d, double(n));
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_obsnorm_apply(amenv_obsnorm* h, const float* in, float* out, int64_t n, float clip, double eps, void* stream) {
  if (!h || !in || !out || n <= 0) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  const int d = h->dim, bs = 256;
  const long long n_elems = (long long)n * d;
  long long blocks = (n_elems + bs - 1) / bs;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(obsnorm_apply_kernel, dim3((unsigned)blocks), dim3(bs), sizeof(double) * 2 * d, (hipStream_t)stream, in, out, n_elems, d, (const double*)h->buf, clip, eps);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_obsnorm_get(amenv_obsnorm* h, double* mean, double* var, double* count, void* stream) {
  if (!h || !mean || !var || !count) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  const int d = h->dim;
  std::string staging(sizeof(double) * (2 * d + 1), '\0');   // one synchronous copy of [mean | var | count]
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(&staging[0], h->buf, staging.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return AMENV_ERR_HIP;
  const double* src = reinterpret_cast<const double*>(staging.data());
  std::memcpy(mean, src, sizeof(double) * d);
  std::memcpy(var, src + d, sizeof(double) * d);
  *count = src[2 * d];
  return AMENV_OK;
}

int amenv_obsnorm_set(amenv_obsnorm* h, const double* mean, const double* var, double count, void* stream) {
  if (!h || !mean || !var) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  const int d = h->dim;
  std::string staging(sizeof(double) * (2 * d + 1), '\0');
  double* dst = reinterpret_cast<double*>(&staging[0]);
  std::memcpy(dst, mean, sizeof(double) * d);
  std::memcpy(dst + d, var, sizeof(double) * d);
  dst[2 * d] = count;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(h->buf, staging.data(), staging.size(), hipMemcpyHostToDevice) != hipSuccess)
    return AMENV_ERR_HIP;
  return AMENV_OK;
}

// ---- reward normaliser (VecNormalize norm_reward; csrc/amenv_retnorm.hpp) ---------------------------------------------
struct amenv_retnorm {
  int64_t n = 0;
  double gamma = 0.0;
  int device = 0;
  double* buf = nullptr;   // retnorm_words(n) doubles on the device: statistics | inv_sigma | returns | partials
};

int amenv_retnorm_create(int64_t num_envs, double gamma, int device, amenv_retnorm** out) {
  if (!out) return fail(nullptr, AMENV_ERR_INVALID, "amenv_retnorm_create: out is NULL");
  if (num_envs <= 0 || num_envs > (int64_t(1) << 31)) return fail(nullptr, AMENV_ERR_INVALID, "amenv_retnorm_create: num_envs must be in 1 .. 2^31");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(nullptr, AMENV_ERR_INVALID, "amenv_retnorm_create: gamma must be in [0, 1]");   // NaN fails the comparison
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(nullptr, AMENV_ERR_NO_DEVICE, "amenv_retnorm_create: no such HIP device");
  amenv_retnorm* h = new (std::nothrow) amenv_retnorm();
  if (!h) return fail(nullptr, AMENV_ERR_ALLOC, "amenv_retnorm_create: out of host memory");
  h->n = num_envs; h->gamma = gamma; h->device = device;
  DeviceGuard g(device);
  const size_t bytes = sizeof(double) * size_t(retnorm_words(num_envs));
  if (hipMalloc((void**)&h->buf, bytes) != hipSuccess) { delete h; return fail(nullptr, AMENV_ERR_ALLOC, "amenv_retnorm_create: hipMalloc failed"); }
  const double init[3] = {0.0, 1.0, 1e-4};   // mean, var, count (sb3 RunningMeanStd defaults)
  if (hipMemset(h->buf, 0, bytes) != hipSuccess || hipMemcpy(h->buf, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(h->buf); delete h;
    return fail(nullptr, AMENV_ERR_HIP, "amenv_retnorm_create: init copy failed");
  }
  *out = h;
  return AMENV_OK;
}

int amenv_retnorm_destroy(amenv_retnorm* h) {
  if (!h) return AMENV_OK;
  { DeviceGuard g(h->device); if (h->buf) (void)hipFree(h->buf); }
  delete h;
  return AMENV_OK;
}

int amenv_retnorm_rollout(amenv_retnorm* h, int32_t n_steps, const float* rewards_in, const uint8_t* dones, float* rewards_out, int32_t update,
                          float clip, double eps, void* stream) {
  if (!h || n_steps <= 0 || !rewards_in || !rewards_out || (update && !dones)) return fail(nullptr, AMENV_ERR_INVALID, "amenv_retnorm_rollout: NULL argument or n_steps <= 0");
  if (!(clip > 0.0f) || !(eps >= 0.0) || !std::isfinite(eps)) return fail(nullptr, AMENV_ERR_INVALID, "amenv_retnorm_rollout: clip must be > 0 and eps finite and >= 0");
  DeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = h->n, waves = retnorm_waves(n);
  for (int32_t t0 = 0; t0 < n_steps; t0 += kRetnormChunk) {   // consecutive chunks: the same bytes as one pass (the header's chunking property)
    const int tc = std::min<int32_t>(kRetnormChunk, n_steps - t0);
    const int64_t o = int64_t(t0) * n;
    if (update) {
      hipLaunchKernelGGL(retnorm_scan_kernel, dim3((unsigned)waves), dim3(64), 0, s, rewards_in + o, dones + o, tc, n, h->gamma,
                         h->buf + retnorm_off_returns(), h->buf + retnorm_off_partials(n));
      hipLaunchKernelGGL(retnorm_merge_kernel, dim3(1), dim3(kRetnormMergeBlock), 0, s, h->buf, tc, n, eps);
    }
    hipLaunchKernelGGL(retnorm_apply_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)tc), dim3(256), 0, s, rewards_in + o, rewards_out + o, n,
                       (const double*)h->buf, update ? 0 : 1, clip, eps);
  }
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_retnorm_reset_returns(amenv_retnorm* h, void* stream) {
  if (!h) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  return hipMemsetAsync(h->buf + retnorm_off_returns(), 0, sizeof(double) * size_t(h->n), (hipStream_t)stream) == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_retnorm_get(amenv_retnorm* h, double* mean, double* var, double* count, double* returns, void* stream) {
  if (!h || !mean || !var || !count) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  double st[3];
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(st, h->buf, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return AMENV_ERR_HIP;
  if (returns && hipMemcpy(returns, h->buf + retnorm_off_returns(), sizeof(double) * size_t(h->n), hipMemcpyDeviceToHost) != hipSuccess) return AMENV_ERR_HIP;
  *mean = st[0]; *var = st[1]; *count = st[2];
  return AMENV_OK;
}

int amenv_retnorm_set(amenv_retnorm* h, double mean, double var, double count, const double* returns, void* stream) {
  if (!h || !std::isfinite(mean) || !(var >= 0.0) || !std::isfinite(var) || !(count > 0.0) || !std::isfinite(count)) return AMENV_ERR_INVALID;
  DeviceGuard g(h->device);
  const double st[3] = {mean, var, count};
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(h->buf, st, sizeof(st), hipMemcpyHostToDevice) != hipSuccess) return AMENV_ERR_HIP;
  if (returns && hipMemcpy(h->buf + retnorm_off_returns(), returns, sizeof(double) * size_t(h->n), hipMemcpyHostToDevice) != hipSuccess) return AMENV_ERR_HIP;
  return AMENV_OK;
}

// Bench / profiling utility: a copy of known size with a chosen access width per lane, so that the PMC traffic counters (FETCH_SIZE,
// WRITE_SIZE) can be calibrated on the access pattern of the kernel under test (16 B per lane: one-lane-per-env kernels; 4 B per lane:
// lane-team kernels) -- /opt/skills/guides/MI355X_MICROARCH.md, HBM section.
int amenv_calibration_copy(const void* src, void* dst, size_t bytes, int32_t bytes_per_lane, void* stream) {
  if (!src || !dst || (bytes_per_lane != 4 && bytes_per_lane != 16) || bytes % 16) return AMENV_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (bytes_per_lane == 4) hipLaunchKernelGGL((calibration_copy_kernel<float>), dim3(2048), dim3(256), 0, s, (const float*)src, (float*)dst, bytes / 4);
  else hipLaunchKernelGGL((calibration_copy_kernel<float4>), dim3(2048), dim3(256), 0, s, (const float4*)src, (float4*)dst, bytes / 16);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

// Right-hand side of the arm vehicle for n states, per-link (form 0) or staged / aggregated (form 1) formulation, fp32 or fp64: the logic gate of
// the arithmetic the stage-wave and lane-team kernels run (tests compare the fp64 instantiation with the oracle's orc_arm_rhs).
int amenv_arm_rhs(const amenv_config* cfg, int32_t form, int32_t dtype, const void* state19, const void* wrench4, const void* cmd3, void* deriv19, int64_t n,
                  void* stream) {
  if (validate(cfg) || cfg->vehicle.n_joints != 3 || cfg->vehicle.n_rotors != 6 || (form != 0 && form != 1) || (dtype != AMENV_F32 && dtype != AMENV_F64) ||
      !state19 || !wrench4 || !cmd3 || !deriv19 || n <= 0)
    return AMENV_ERR_INVALID;
  if (generic_axes(cfg->vehicle)) return AMENV_ERR_INVALID;   // z,x,x arm
  amenv tmp;
  tmp.cfg = *cfg;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AMENV_F64) {
    const HotParams<double, 6> P = make_hot<double, 6>(tmp);
    const ArmParams<double> A = make_arm<double>(tmp);
    if (form == 0) hipLaunchKernelGGL((arm_rhs_kernel<double, 0, HotParams<double, 6>>), grid, block, 0, s, P, A, (const double*)state19, (const double*)wrench4, (const double*)cmd3, (double*)deriv19, (int64_t)n);
    else hipLaunchKernelGGL((arm_rhs_kernel<double, 1, HotParams<double, 6>>), grid, block, 0, s, P, A, (const double*)state19, (const double*)wrench4, (const double*)cmd3, (double*)deriv19, (int64_t)n);
  } else {
    const HotParams<float, 6> P = make_hot<float, 6>(tmp);
    const ArmParams<float> A = make_arm<float>(tmp);
    if (form == 0) hipLaunchKernelGGL((arm_rhs_kernel<float, 0, HotParams<float, 6>>), grid, block, 0, s, P, A, (const float*)state19, (const float*)wrench4, (const float*)cmd3, (float*)deriv19, (int64_t)n);
    else hipLaunchKernelGGL((arm_rhs_kernel<float, 1, HotParams<float, 6>>), grid, block, 0, s, P, A, (const float*)state19, (const float*)wrench4, (const float*)cmd3, (float*)deriv19, (int64_t)n);
  }
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

// ---- PID + minimum-snap baseline controller (row f4; csrc/amenv_baseline.hpp) ---------------------------------------------------------
int amenv_pid_default_params(amenv_pid_params* p) {
  if (!p) return AMENV_ERR_INVALID;
  static const double kGains[18] = {3.0, 30.0, 1.0, 3.0, 30.0, 1.0, 1000.0, 200.0, 10.0,      // x, y, z       (pid_controller.py:16-18)
                                    160.0, 3.0, 1.0, 160.0, 3.0, 1.0, 80.0, 5.0, 1.0};        // phi theta psi (:19-21)
  p->dt = 0.01; p->mass = 0.18; p->g = 9.81; p->max_integral = 100.0;
  std::memcpy(p->gain, kGains, sizeof(kGains));
  return AMENV_OK;
}

namespace {
bool pid_params_ok(const amenv_pid_params* p) { return p && p->dt > 0.0 && p->mass > 0.0 && p->g > 0.0 && p->max_integral >= 0.0; }
PidParams to_dev(const amenv_pid_params& p) {
  PidParams d;
  d.dt = p.dt; d.mass = p.mass; d.g = p.g; d.max_integral = p.max_integral;
  for (int k = 0; k < 6; k++) for (int j = 0; j < 3; j++) d.gain[k][j] = p.gain[3 * k + j];
  return d;
}
}  // namespace

int amenv_pid_run(const amenv_pid_params* p, int32_t dtype, const void* state, const void* des, void* integral, void* F_out, void* M_out,
                  void* rpy_out, int64_t n, void* stream) {
  if (!pid_params_ok(p) || !state || !des || !integral || !F_out || !M_out || n <= 0 || (dtype != AMENV_F32 && dtype != AMENV_F64)) return AMENV_ERR_INVALID;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  const PidParams d = to_dev(*p);
  if (dtype == AMENV_F64)
    hipLaunchKernelGGL(pid_run_kernel<double>, grid, block, 0, (hipStream_t)stream, d, (const double*)state, (const double*)des, (double*)integral,
                       (double*)F_out, (double*)M_out, (double*)rpy_out, (int64_t)n);
  else
    hipLaunchKernelGGL(pid_run_kernel<float>, grid, block, 0, (hipStream_t)stream, d, (const float*)state, (const float*)des, (float*)integral,
                       (float*)F_out, (float*)M_out, (float*)rpy_out, (int64_t)n);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

size_t amenv_minsnap_workspace_bytes(int32_t n_segments) {
  return (n_segments < 1 || n_segments > 16) ? 0 : size_t(8 * n_segments) * size_t(10 * n_segments) * sizeof(double);
}

int amenv_minsnap_solve(int32_t n_segments, int64_t n_traj, double speed, const double* waypoints, double* coeff, double* seg_time,
                        double* seg_start, void* workspace, void* stream) {
  if (n_segments < 1 || n_segments > 16 || n_traj <= 0 || !(speed > 0.0) || !waypoints || !coeff || !seg_time || !seg_start || !workspace)
    return AMENV_ERR_INVALID;
  hipLaunchKernelGGL(minsnap_inverse_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)n_segments, (double*)workspace);
  const int64_t rows = n_traj * 8 * n_segments;
  hipLaunchKernelGGL(minsnap_coeff_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)n_segments, (int64_t)n_traj,
                     speed, (const double*)workspace, waypoints, coeff, seg_time, seg_start);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_minsnap_eval(int32_t n_segments, int64_t n_query, const double* coeff, const double* seg_time, const double* seg_start,
                       const double* waypoints, const int64_t* traj, const double* t, int32_t dtype, void* des, void* stream) {
  if (n_segments < 1 || n_segments > 16 || n_query <= 0 || !coeff || !seg_time || !seg_start || !waypoints || !t || !des ||
      (dtype != AMENV_F32 && dtype != AMENV_F64))
    return AMENV_ERR_INVALID;
  const dim3 grid((unsigned)((n_query + 63) / 64)), block(64);
  if (dtype == AMENV_F64)
    hipLaunchKernelGGL(minsnap_eval_kernel<double>, grid, block, 0, (hipStream_t)stream, (int)n_segments, (int64_t)n_query, coeff, seg_time, seg_start,
                       waypoints, traj, t, (double*)des);
  else
    hipLaunchKernelGGL(minsnap_eval_kernel<float>, grid, block, 0, (hipStream_t)stream, (int)n_segments, (int64_t)n_query, coeff, seg_time, seg_start,
                       waypoints, traj, t, (float*)des);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_pid_policy(const amenv_pid_policy_params* p, int32_t dtype, const float* obs, const uint8_t* done, void* pstate, float* actions,
                     int64_t n, void* stream) {
  if (!p || !pid_params_ok(&p->pid) || !obs || !pstate || !actions || n <= 0 || (dtype != AMENV_F32 && dtype != AMENV_F64) || !(p->speed > 0.0) ||
      !(p->moment_scale > 0.0) || p->obs_dim < 20 || p->act_dim < 4 || p->act_dim > 16 || (p->tool_mode != 0 && p->obs_dim < 23))
    return AMENV_ERR_INVALID;
  PidPolicyParams d;
  d.pid = to_dev(p->pid);
  d.speed = p->speed; d.moment_scale = p->moment_scale;
  for (int k = 0; k < 3; k++) d.m_gain[k] = p->inertia_ratio[k];
  d.obs_dim = p->obs_dim; d.act_dim = p->act_dim; d.tool_mode = p->tool_mode ? 1 : 0; d.pad = 0;
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  if (dtype == AMENV_F64) hipLaunchKernelGGL(pid_policy_kernel<double>, grid, block, 0, (hipStream_t)stream, d, obs, done, (double*)pstate, actions, (int64_t)n);
  else hipLaunchKernelGGL(pid_policy_kernel<float>, grid, block, 0, (hipStream_t)stream, d, obs, done, (float*)pstate, actions, (int64_t)n);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

}  // extern "C"
