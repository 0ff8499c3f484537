// amenv_host.hpp -- what more than one source of libamenv.so needs on the host: the handle, the parameter packers, the compile-time
// visitors and the predicates over a config.  Internal: every amenv_capi*.hip includes it, nothing outside csrc/ does.  Templates and
// one-line helpers sit in an anonymous namespace (each source gets its own copy); a function that owns state, or is too large to want
// a copy per source, is DEFINED once in amenv_capi.hip and only declared here, hidden from the library's exports.
// Every kernel is compiled in exactly one source: this header includes kernel TEMPLATES only, never a header that defines a
// non-template __global__ function.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "amenv_kernels.hpp"
#include "amenv_team.hpp"
#include "amenv_team_host.hpp"
#include "amenv_quad.hpp"
#include "amenv_policy_mlp.hpp"

using namespace amenv_dev;

// which step kernel amenv_step runs (select_step_family); amenv_rollout runs the family's own rollout kernel where it has one
enum class StepFamily {
  Lane,         // step_kernel: one lane per env
  LaneHelper,   // step_kernel_pw: rigid vehicles at small batches, helper waves per tile (reset RNG words, observation rows, Monitor totals)
  Quad,         // step_kernel_quad: rigid vehicles, 4 lanes per env (amenv_quad.hpp); opt-in
  Team,         // step_kernel_team: z,x,x-arm vehicle in the latency regime, 16 lanes per env (amenv_team.hpp); fp64 = logic-gate build
  Staged,       // step_kernel_armk: z,x,x-arm vehicle, four RK4 stage waves + a main wave per 64-env tile; fp64 = logic-gate build
  TwoWave,      // step_kernel_arm2w: fp32 z,x,x-arm vehicle, main + helper wave per 64-env tile
};

struct amenv {
  amenv_config cfg;
  int device = -1;
  int obs_dim = 20, act_dim = kActDim, nf = 0;
  void* blob = nullptr;            // tiled episode state (amenv_kernels.hpp "Data layout")
  unsigned long long* stats = nullptr;
  size_t blob_bytes = 0, fbytes = 0, ibytes = 0;
  uint32_t tile_bytes = 0;
  int n_tiles = 0;
  int block = 64;
  StepFamily family = StepFamily::Lane;
  void* team_consts = nullptr;     // per-lane constants of the team / quad kernels (amenv_team_host.hpp): float4 pieces, or plain doubles for the fp64 build
  uint32_t* pol_pack = nullptr;    // amenv_rollout_policy: policy parameters as MFMA fragments (re-packed on every call)
  // n-link arm with n < 3 (amenv_vehicle.n_joints = 1 or 2): inside, the vehicle is the 3-joint one with PHANTOM links behind the real ones (zero
  // mass / inertia / offset, joint limits 0 -> command 0, state 0: every term they add is an exact zero), so every kernel family serves it;
  // the C ABI keeps the caller's dimensions (4 + n actions, 20 + 2 n + 3 observations, 2 n joint fields): pack / unpack kernels at the boundary
  int pub_nj = 0;                  // the caller's n_joints (cfg.vehicle.n_joints is the internal 3 when this is 1 or 2)
  float* io_act = nullptr;         // [N][7]   padded actions
  float* io_obs = nullptr;         // [N][29]  internal observation rows
  float* io_term = nullptr;        // [N][29]  internal terminal-observation rows
  uint64_t steps = 0;
  bool dr = false;                 // amenv_set_randomization: per-episode dynamics randomisation on
  DrRanges dr_r = {{1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f}};   // its ranges (lo, hi - lo); {1, 1} = the nominal vehicle
  bool lag = false;                // amenv_set_rotor_lag: first-order rotor lag on
  double lag_a[2] = {1.0, 1.0};    // its coefficients -expm1(-dt / tau_up), -expm1(-dt / tau_down), fp64
  bool noise = false;              // amenv_set_sensor_noise: sensor noise on the observation rows
  NoiseSig noise_s = {0.0f, 0.0f, 0.0f, 0.0f};   // its standard deviations: position, velocity, body rate, attitude
  void* lag_w = nullptr;           // [n_tiles][n_rotors][64] rotor states | [n_rotors] w0, of the handle's dtype; allocated when the lag is first enabled
  bool delay = false;              // amenv_set_action_delay: per-episode actuation latency on
  int32_t delay_lo = 0, delay_hi = 0;   // its range of control steps, for the episodes that start from now on
  void* delay_h = nullptr;         // float4 [n_tiles][8][64] given rows | int32 [n_tiles * 64] d | head << 4; allocated when the delay or the history is first enabled
  int hist = 0;                    // amenv_set_action_history: given action rows appended to every observation row, 0..2; > 0 runs the DELAY kernels
  float* hist_obs = nullptr;       // [N][obs_dim] the task's rows of amenv_reset / amenv_observe while the history is on, widened into the caller's buffer
  RateBlock rate = {0, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};   // amenv_set_rate_control: body-rate actions; on = 0: off
  FailBlock fail = {0u, 0u, 0u, 0.0f, 0.0f};   // amenv_set_rotor_failure: per-episode rotor failure; ctl = 0: off
  bool delay_path() const { return delay || hist > 0; }   // the DELAY instantiations run: the latency, the history (range (0, 0) without the latency) or both
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // amenv_step_timed only
  std::string err;
  mutable std::string kname;       // amenv_kernel_name forms it from the state above when it is asked for
};

// amenv_obsnorm_* (amenv_capi.hip); amenv_rollout_policy_norm and amenv_evaluate_policy read its buffer
struct amenv_obsnorm {
  int dim = 0, device = 0;
  double* buf = nullptr;   // obsnorm_words(dim) doubles on the device
};

// ---- defined once, in amenv_capi.hip ----------------------------------------------------------------------------------------------
// records msg in the handle (e null: in the calling thread's amenv_create error) and returns code
__attribute__((visibility("hidden"))) int fail(amenv* e, int code, const std::string& msg);
// Lane-team step kernel: four integrating waves + one helper per workgroup while every workgroup gets a CU to itself, else one + one
// (amenv_team.hpp, step_kernel_team).
__attribute__((visibility("hidden"))) bool team_wide(const amenv& e);
// amenv_kernel_name: tests, tools/ and bench.py match substrings of it
__attribute__((visibility("hidden"))) std::string kernel_name(const amenv& e);
// Which step kernel a config runs: amenv_config.step_kernel, or by batch size for AUTO (crossovers measured on MI355X).
// Returns the refusal text when a requested kernel is not built for the config.
__attribute__((visibility("hidden"))) const char* select_step_family(const amenv_config& c, StepFamily* out);
// amenv_rollout_policy[_norm] after the entry checks: pack the parameters, fill the kernel's I/O block
// (the one place that launches policy_pack_kernel)
__attribute__((visibility("hidden"))) PolicyIO policy_io(amenv& e, const float* flat_params, uint64_t seed, uint32_t draw0, float* obs, float* actions, float* logp, float* values, float* rewards,
                   uint8_t* dones, uint32_t* info_bits, float* terminal_obs, hipStream_t s);
// n-link arm, n < 3: the boundary adapters (see struct amenv); their kernels sit in amenv_capi.hip
__attribute__((visibility("hidden"))) hipError_t pad_actions(const amenv& e, const float* actions, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t cut_obs(const amenv& e, const float* rows29, const uint8_t* rows_of, float* out, hipStream_t s);

namespace {

struct DeviceGuard {
  int prev = -1, dev;
  explicit DeviceGuard(int d) : dev(d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
  }
};

#define AMENV_HIP(e, call)                                                                       \
  do {                                                                                           \
    hipError_t _s = (call);                                                                      \
    if (_s != hipSuccess) return fail(e, AMENV_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s)); \
  } while (0)

template <typename T, int NR>
HotParams<T, NR> make_hot(const amenv& e) {
  const amenv_config& c = e.cfg;
  const amenv_vehicle& v = c.vehicle;
  HotParams<T, NR> P;
  std::memset(&P, 0, sizeof(P));
  for (int r = 0; r < v.n_rotors; r++) {
    for (int j = 0; j < 4; j++) P.alloc[r][j] = T(v.alloc[r * 4 + j]);
    for (int j = 0; j < 3; j++) P.mixm[j][r] = T(v.mix[(1 + j) * v.n_rotors + r]);
    P.tmin[r] = T(v.t_min[r]); P.tmax[r] = T(v.t_max[r]);
  }
  const double* I = v.inertia; const double* J = v.inv_inertia;
  P.Ixx = T(I[0]); P.Ixy = T(I[1]); P.Ixz = T(I[2]); P.Iyy = T(I[4]); P.Iyz = T(I[5]); P.Izz = T(I[8]);
  P.Jxx = T(J[0]); P.Jxy = T(J[1]); P.Jxz = T(J[2]); P.Jyy = T(J[4]); P.Jyz = T(J[5]); P.Jzz = T(J[8]);
  const int ns = c.task.rk4_substeps > 0 ? c.task.rk4_substeps : 1;
  P.inv_mass = T(1.0 / v.mass); P.g = T(v.g); P.h = T(c.task.dt / ns);
  P.mass_f = float(v.mass); P.g_f = float(v.g); P.mscale_f = float(v.moment_scale);
  P.n_rotors = v.n_rotors; P.substeps = ns;
  P.max_steps = c.task.max_episode_steps; P.counter_limit = c.task.counter_limit;
  P.flags = c.flags; P.K = c.task.num_waypoints; P.raw_obs = c.task.variant == AMENV_TASK_V1_RAW17 ? 1 : 0;
  P.ee_task = (v.n_joints > 0 && c.task.ee_task == AMENV_EE_TASK_TOOL) ? 1 : 0;
  return P;
}

// joint axes other than (z, x, x): the kernels take the general-axes body, and only the lane kernel serves them
bool generic_axes(const amenv_vehicle& v) {
  const double zxx[9] = {0, 0, 1, 1, 0, 0, 1, 0, 0};
  return std::memcmp(v.joint_axis, zxx, sizeof(zxx)) != 0;
}

template <typename T>
ArmParams<T> make_arm(const amenv& e) {
  const amenv_vehicle& v = e.cfg.vehicle;
  ArmParams<T> A;
  std::memset(&A, 0, sizeof(A));
  for (int k = 0; k < 3; k++) {
    for (int c = 0; c < 3; c++) { A.jo[k][c] = T(v.joint_origin[3 * k + c]); A.ja[k][c] = T(v.joint_axis[3 * k + c]); A.lc[k][c] = T(v.link_com[3 * k + c]); }
    A.lm[k] = T(v.link_mass[k]);
    const double* I = &v.link_inertia[9 * k];
    A.li[k][0] = T(I[0]); A.li[k][1] = T(I[1]); A.li[k][2] = T(I[2]); A.li[k][3] = T(I[4]); A.li[k][4] = T(I[5]); A.li[k][5] = T(I[8]);
    const float lo = float(v.joint_limit[2 * k]), hi = float(v.joint_limit[2 * k + 1]);
    A.half[k] = 0.5f * (hi - lo); A.mid[k] = 0.5f * (hi + lo);

  }
  A.kp = T(v.joint_kp); A.kd = T(v.joint_kd); A.amax = T(v.joint_acc_max);
  A.generic_axes = generic_axes(v) ? 1 : 0;
  A.mtot = T(v.mass); A.inv_mtot = T(1.0 / v.mass);
  for (int c = 0; c < 3; c++) {
    A.tool[c] = T(v.tool_offset[c]);
    // arm at home: every joint rotation is the identity, whatever the axes
    A.ee_home[c] = v.n_joints > 0 ? T(v.joint_origin[c] + v.joint_origin[3 + c] + v.joint_origin[6 + c] + v.tool_offset[c]) : T(0);
  }
  return A;
}

// per-lane constant table / wave-uniform parameters of the team kernels: amenv_team_host.hpp (shared with the host emulation of tests/emu)
template <typename T> TeamParamsT<T> make_team(const amenv& e) { return make_team_params<T>(e.cfg, e.team_consts); }
QuadParams make_quad(const amenv& e) {
  const amenv_config& c = e.cfg;
  const amenv_vehicle& v = c.vehicle;
  QuadParams P;
  std::memset(&P, 0, sizeof(P));
  const int six[6] = {0, 1, 2, 4, 5, 8};
  for (int j = 0; j < 6; j++) { P.I[j] = float(v.inertia[six[j]]); P.Iinv[j] = float(v.inv_inertia[six[j]]); }
  P.inv_mass = float(1.0 / v.mass);
  const int ns = c.task.rk4_substeps > 0 ? c.task.rk4_substeps : 1;
  P.h = float(c.task.dt / ns); P.substeps = ns;
  for (int r = 0; r < 6 && r < v.n_rotors; r++) { P.tmin[r] = float(v.t_min[r]); P.tmax[r] = float(v.t_max[r]); }
  P.max_steps = c.task.max_episode_steps; P.counter_limit = c.task.counter_limit; P.flags = c.flags;
  P.ee_task = 0; P.K = 1;
  P.consts = reinterpret_cast<const float4*>(e.team_consts);
  return P;
}

ColdParams make_cold(const amenv& e) {
  const amenv_config& c = e.cfg;
  ColdParams C;
  for (int k = 0; k < AMENV_MAX_WAYPOINTS; k++) { C.traj_sin[k] = float(c.task.traj_sin[k]); C.traj_cos[k] = float(c.task.traj_cos[k]); }
  C.seed_lo = uint32_t(c.seed); C.seed_hi = uint32_t(c.seed >> 32);
  C.gid0 = c.env_id_offset;
  return C;
}

template <typename T, int NROT> LagArg<T, NROT, true> make_lag(const amenv& e) {
  LagArg<T, NROT, true> L;
  L.w = static_cast<T*>(e.lag_w); L.n_pad = uint32_t(e.n_tiles) * 64u;
  L.a_up = T(e.lag_a[0]); L.a_down = T(e.lag_a[1]);
  return L;
}
DelayArg<true> make_delay(const amenv& e) {
  DelayArg<true> D;
  D.h = static_cast<float4*>(e.delay_h); D.n_pad = uint32_t(e.n_tiles) * 64u;
  D.lo = e.delay ? e.delay_lo : 0; D.span = e.delay ? e.delay_hi - e.delay_lo + 1 : 1;   // the history alone: range (0, 0), every d is 0
  D.hist = e.hist;
  return D;
}
// the kernels' last argument: the randomisation ranges, behind them the lag block in the LAG instantiations, behind that the sensor
// noise's sigmas in the NOISE ones, behind those the actuation latency's fields in the DELAY ones
template <typename T, int NROT, unsigned DYN> DynArg<T, NROT, DYN> make_dyn(const amenv& e) {
  DynArg<T, NROT, DYN> a;
  if constexpr ((DYN & kDynDr) != 0) { a.R.r = e.dr_r; a.R.q = e.rate; a.R.x = e.fail; } else a.R.unused = 0;
  if constexpr ((DYN & kDynLag) != 0) a.L = make_lag<T, NROT>(e);
  if constexpr ((DYN & kDynNoise) != 0) a.Z.s = e.noise_s;
  if constexpr ((DYN & kDynDelay) != 0) a.D = make_delay(e);
  return a;
}
// the cold kernels' (reset, observe) runtime switch
NoiseRt make_noise_rt(const amenv& e) {
  return NoiseRt{e.noise_s, uint32_t(e.cfg.seed), uint32_t(e.cfg.seed >> 32), e.cfg.env_id_offset, e.noise ? 1 : 0};
}

bool is_v1(const amenv_config* c) { return c->task.variant == AMENV_TASK_V1_SCALED17 || c->task.variant == AMENV_TASK_V1_RAW17; }

// The predicates below take the internal config: validated (an arm implies 6 rotors and the v2 task) and padded (an arm of 1 or 2 joints has
// n_joints = 3, pad_arm_config).
// z,x,x arm on the single-waypoint task: the team, stage-wave and two-wave kernels
bool zxx_arm1(const amenv_config& c) { return c.vehicle.n_joints == 3 && !generic_axes(c.vehicle) && c.task.num_waypoints == 1; }
// lane-quad kernels (step: opt-in; closed loop: amenv_rollout_policy): fp32 rigid vehicle with 4 or 6 rotors, single-waypoint v2 task, default workgroup size
bool quad_ok(const amenv_config& c) {
  return c.vehicle.n_joints == 0 && c.dtype == AMENV_F32 && (c.vehicle.n_rotors == 4 || c.vehicle.n_rotors == 6) && !is_v1(&c) && c.task.num_waypoints == 1 &&
         c.block_size == 0;
}
// fp32 lane-team kernels (step, rollout, closed loop: amenv_rollout_policy)
bool team_ok(const amenv_config& c) { return c.dtype == AMENV_F32 && zxx_arm1(c); }
// one-lane-per-env closed loop of the rigid vehicles (amenv_rigid_policy.hpp): fp32, 4 or 6 rotors, every task, any workgroup size
bool rigid_pol_ok(const amenv_config& c) { return c.vehicle.n_joints == 0 && c.dtype == AMENV_F32 && (c.vehicle.n_rotors == 4 || c.vehicle.n_rotors == 6); }
// closed loop (amenv_rollout_policy) of an fp32 arm vehicle: every one of them -- 1..3 joints (the internal, phantom-padded config has 3),
// 1..4 waypoints, any joint axes.  The team kernel where the step runs it (team_ok, family Team), the lane form (amenv_lane_policy.hpp) elsewhere
bool arm_pol_ok(const amenv_config& c) { return c.vehicle.n_joints == 3 && c.dtype == AMENV_F32; }

// one kernel launch; timed: stamped at dispatch and completion with amenv_step_timed's events
template <typename... P, typename... A>
hipError_t launch(const amenv& e, bool timed, void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
  if (timed) hipExtLaunchKernelGGL(k, grid, block, lds, s, e.ev_start, e.ev_stop, 0, args...);
  else hipLaunchKernelGGL(k, grid, block, lds, s, args...);
  return hipGetLastError();
}

// The switch set a handle runs, for amenv_step, amenv_rollout and the closed-loop rollouts alike: the lag, the noise and the DELAY path, and DR with any
// of them, with rate control or with the rotor failure, whose blocks travel with the ranges (unit ranges when randomisation is off).  The setters admit rigid vehicles with 4 or 6 rotors only: every other handle runs the kernels without switches (a switch on such a handle, which no setter lets happen, would be dropped here, not refused).
unsigned dyn_set(const amenv& e) {
  const int nr = e.cfg.vehicle.n_rotors;
  if (e.cfg.vehicle.n_joints > 0 || (nr != 4 && nr != 6)) return 0;
  const unsigned on = (e.lag ? kDynLag : 0) | (e.noise ? kDynNoise : 0) | (e.delay_path() ? kDynDelay : 0);
  return on | (on || e.dr || e.rate.on || e.fail.ctl ? kDynDr : 0);
}
template <auto V> using const_c = std::integral_constant<decltype(V), V>;
// f(const_c<NROT>, const_c<DYN>) with DYN == dyn, over the sets that are built for T (dyn_admitted) and NROT (the general rotor count: no switch)
template <typename T, int NROT, unsigned DYN = 0, typename F>
hipError_t with_dyn(unsigned dyn, F& f) {
  if constexpr (DYN <= kDynAll) {
    if constexpr (dyn_admitted<T, 0>(DYN) && (DYN == 0 || NROT == 4 || NROT == 6)) { if (dyn == DYN) return f(const_c<NROT>{}, const_c<DYN>{}); }
    return with_dyn<T, NROT, DYN + 1>(dyn, f);
  }
  return hipErrorInvalidValue;
}
// a rigid handle's compile-time form: its rotor count (4, 6, or the general loop bound) and its switch set
template <typename T, typename F>
hipError_t with_rigid_form(const amenv& e, F f) {
  const unsigned dyn = dyn_set(e);
  const int nr = e.cfg.vehicle.n_rotors;
  return nr == 4 ? with_dyn<T, 4>(dyn, f) : nr == 6 ? with_dyn<T, 6>(dyn, f) : with_dyn<T, AMENV_MAX_ROTORS>(dyn, f);
}
// a rigid handle's task: f(const_c<KW>, const_c<VAR>)
template <typename F>
hipError_t with_task(const amenv& e, F f) {
  if (is_v1(&e.cfg)) return f(const_c<2>{}, const_c<VAR_V1>{});   // v1: up to 2 waypoints per episode
  if (e.cfg.task.num_waypoints == 1) return f(const_c<1>{}, const_c<VAR_V2>{});
  return f(const_c<AMENV_MAX_WAYPOINTS>{}, const_c<VAR_V2>{});
}
// the kernels built for 4 and 6 rotors alone (the caller has refused every other count): f(const_c<NROT>)
template <typename F>
auto with_rotors46(int nr, F f) { return nr == 4 ? f(const_c<4>{}) : f(const_c<6>{}); }

// The (obs_dim, act_dim) pairs the policy kernels are built for (amenv_policy_forward, amenv_policy_forward_mfma, amenv_ppo_mlp_step), stated once here
// for the library; ActorCritic._FUSED_DIMS (ppo.py) and the comments in include/amenv.h name the same nine, tests/test_gpu_policy_shapes.py holds them together
template <int D, int A> struct shape_c {};
template <typename... S> struct shape_list {};
using PolicyShapes = shape_list<shape_c<20, 4>, shape_c<29, 7>, shape_c<17, 4>, shape_c<25, 5>, shape_c<27, 6>,   // v2 | hexacopter + 3-link arm | v1 | hexacopter + 1- / 2-link arm
                                shape_c<24, 4>, shape_c<28, 4>, shape_c<21, 4>, shape_c<25, 4>>;                  // v2 / v1 rows of the rigid vehicles with one or two action rows of history
// the action widths amenv_gaussian_act and amenv_ppo_loss_grad are built for: 4 = quad / hexa, 4 + n = hexa + n joints (the rows' width plays no part: 0)
using ActionWidths = shape_list<shape_c<0, 4>, shape_c<0, 5>, shape_c<0, 6>, shape_c<0, 7>>;
// f(const_c<D>, const_c<A>) for the listed pair that equals (d, a); hipErrorInvalidValue when none does
template <typename F, int... D, int... A>
hipError_t with_shape(shape_list<shape_c<D, A>...>, int d, int a, const F& f) {
  hipError_t st = hipErrorInvalidValue;
  (void)((d == D && a == A && (st = f(const_c<D>{}, const_c<A>{}), true)) || ...);
  return st;
}
template <typename F> hipError_t with_policy_shape(int obs_dim, int act_dim, const F& f) { return with_shape(PolicyShapes{}, obs_dim, act_dim, f); }
template <typename F> hipError_t with_act_dim(int act_dim, const F& f) { return with_shape(ActionWidths{}, 0, act_dim, [&](auto, auto a) { return f(a); }); }
bool policy_shape_built(int obs_dim, int act_dim) { return with_policy_shape(obs_dim, act_dim, [](auto, auto) { return hipSuccess; }) == hipSuccess; }
bool act_dim_built(int act_dim) { return with_act_dim(act_dim, [](auto) { return hipSuccess; }) == hipSuccess; }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
