// amenv_model.hpp -- per-environment device code for gfx950 (CDNA4): everything one lane does
// for one environment in one control step.  One lane = one environment; all of an
// environment's episode state lives in that lane's registers for the whole step.
//
// Semantics follow the reference (paths relative to the reference root,
// v2 = initial-implementation-v2):
//   mixer / clamp / re-mix        v2/simul_files/model/quadcopter.py:105-112
//   ODE right-hand side           v2/simul_files/model/quadcopter.py:66-103
//   R(q/|q|) third column         v2/simul_files/utils/quaternion.py:46-77 (closed form)
//   integrate + renormalise       v2/simul_files/model/quadcopter.py:113-114 (RK4 for odeint)
//   reward                        v2/rl_env_scaledObs.py:198-231
//   step state machine            v2/rl_env_scaledObs.py:135-196
//   observation                   v2/rl_env_scaledObs.py:98-121
//   quaternion -> roll/pitch/yaw  v2/utils2/utils.py:4-9
//   reset + waypoint generators   v2/rl_env_scaledObs.py:40-79, v2/utils2/utils.py:12-95
//
// Templated on the arithmetic type T: float is the product path, double is the logic-check
// build of the SAME code (tests compare it with the fp64 CPU oracle at ~1e-12).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/amenv.h"

namespace amenv_dev {

constexpr int kActDim = 4;
enum TaskVar { VAR_V2 = 0, VAR_V1 = 1 };                 // v2/rl_env_scaledObs.py | v1/rl_env_scaledObs.py + v1/rl_env.py
// v2 + arm: + joint angle, rate per joint + (tool point - base position) / 0.5 in world axes (forward kinematics)
template <int VAR, int NJ = 0> struct ObsDim { static constexpr int value = VAR == VAR_V1 ? 17 : 20 + 2 * NJ + (NJ > 0 ? 3 : 0); };
constexpr int kObsDimMax = 29;

// ---- kernel-argument constants (uniform: they live in SGPRs) ----------------------------------
// Hot parameters are kept COMPACT (rotor-count-sized mixer, symmetric inertia) so that one batch of
// scalar loads at kernel entry brings all of them into the ~100 available SGPRs: with 64 lone
// wavefronts per launch every extra dependent scalar-load phase is ~0.3 us of pure latency.
template <typename T, int NR>
struct HotParams {
  T alloc[NR][4];   // rotor thrusts = alloc . [F,Mx,My,Mz]            (quadcopter.py:109)
  T mixm[3][NR];    // [Mx,My,Mz] = mixm . thrusts; F = sum(thrusts)    (quadcopter.py:111-112)
  T tmin[NR], tmax[NR];
  T Ixx, Ixy, Ixz, Iyy, Iyz, Izz;   // inertia (symmetric)
  T Jxx, Jxy, Jxz, Jyy, Jyz, Jzz;   // inverse inertia (symmetric)
  T inv_mass, g, h;                 // h = dt / substeps
  float mass_f, g_f, mscale_f;      // action scaling is fp32 in the reference (NumPy >= 2 promotion)
  int32_t n_rotors;                 // used only by the generic (NR = AMENV_MAX_ROTORS) instantiation
  int32_t substeps, max_steps, counter_limit;
  uint32_t flags;
  int32_t K;                        // waypoints per episode (<= KW of the instantiation); v1: storage bound
  int32_t raw_obs;                  // v1 only: 1 = v1/rl_env.py (unscaled observation)
  int32_t ee_task;                  // arm vehicles: 1 = the waypoint task measures from the tool point (AMENV_EE_TASK_TOOL)
};

// Parameters only the reset path needs (cold: loaded when a lane actually resets).
struct ColdParams {
  float traj_sin[AMENV_MAX_WAYPOINTS], traj_cos[AMENV_MAX_WAYPOINTS];
  uint32_t seed_lo, seed_hi;
  int64_t gid0;                     // global id of local env 0
};

// ---- math helpers: one definition per arithmetic type ------------------------------------
__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }   // 1 ulp, 1 instr
__device__ __forceinline__ double rcp_(double x) { return 1.0 / x; }
__device__ __forceinline__ float sqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }  // v_sqrt_f32, 1 ulp, 1 instr
__device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
__device__ __forceinline__ float rsqrt_(float x) {                                     // v_rsq + one Newton step
  float y = __builtin_amdgcn_rsqf(x);
  return y * __builtin_fmaf(-0.5f * x, y * y, 1.5f);
}
__device__ __forceinline__ double rsqrt_(double x) { return 1.0 / sqrt(x); }
// fp32 atan2 / asin for the hold-phase bonuses (rl_env_scaledObs.py:163,169-171).  The device libm versions cost
// ~430 cycles each for a lone wavefront and the hold phase is where a trained policy spends ~500 steps per episode,
// so they are replaced by a compact form: octant reduction + the cephes atanf minimax polynomial on |t| <= tan(pi/8)
// (abs error <= 3e-7 rad incl. the two v_rcp_f32; the bonuses scale angles by <= 50, far inside the 1e-5 gate).
__device__ __forceinline__ float atan_reduced_(float t) {  // |t| <= 0.41421356
  const float z = t * t;
  float p = __builtin_fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
  p = __builtin_fmaf(p, z, 1.99777106478e-1f);
  p = __builtin_fmaf(p, z, -3.33329491539e-1f);
  return __builtin_fmaf(p * z, t, t);
}
__device__ __forceinline__ float atan2_(float y, float x) {
  const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  const bool swap = ay > ax;
  const float mx = swap ? ay : ax, mn = swap ? ax : ay;
  const float t = mn * __builtin_amdgcn_rcpf(mx);                       // [0, 1]
  const bool big = t > 0.41421356237f;
  const float tr = big ? (t - 1.0f) * __builtin_amdgcn_rcpf(t + 1.0f) : t;
  float a = atan_reduced_(tr);
  a = big ? a + 0.78539816339744831f : a;
  a = swap ? 1.57079632679489662f - a : a;
  a = x < 0.0f ? 3.14159265358979324f - a : a;
  a = mx == 0.0f ? 0.0f : a;
  return __builtin_copysignf(a, y);
}
__device__ __forceinline__ double atan2_(double a, double b) { return atan2(a, b); }
__device__ __forceinline__ float asin_(float a) { return atan2_(a, __builtin_amdgcn_sqrtf((1.0f - a) * (1.0f + a))); }
__device__ __forceinline__ double asin_(double a) { return asin(a); }
__device__ __forceinline__ float clamp_(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }  // v_med3_f32
__device__ __forceinline__ double clamp_(double x, double lo, double hi) { return __builtin_fmax(__builtin_fmin(x, hi), lo); }
__device__ __forceinline__ float abs_(float a) { return fabsf(a); }
__device__ __forceinline__ double abs_(double a) { return fabs(a); }
__device__ __forceinline__ bool finite_(float a) { return __builtin_isfinite(a); }
__device__ __forceinline__ bool finite_(double a) { return __builtin_isfinite(a); }
// AMENV_FLAG_NAN_GUARD, case (b): +0 for a finite action entry, NaN for a NaN or an infinite one (no overflow, whatever its size).  The
// marks of a row are summed and the sum joins the state sum the guard tests: the rotor clamp and the joint servo's acceleration limit
// swallow a non-finite entry, so the state after the dynamics need not show it.
__device__ __forceinline__ float nonfinite_mark(float a) { return a * 0.0f; }
__device__ __forceinline__ double nonfinite_mark(double a) { return a * 0.0; }
template <typename T> struct NoActionMark { __device__ __forceinline__ T operator()() const { return T(0); } };

// ---- per-env registers ------------------------------------------------------------------------
template <typename T, int KW>
struct Env {
  T px, py, pz, vx, vy, vz, qw, qx, qy, qz, wx, wy, wz;
  T wp[KW][3];
  T final_yaw, last_distance, ep_return;
  T th[AMENV_MAX_JOINTS], thd[AMENV_MAX_JOINTS];   // arm joint angles / rates (unused, and eliminated, without an arm)
  T eox, eoy, eoz;                                 // arm: tool point - base position, world axes (forward kinematics of the post-step
                                                   // state; derived, not stored)
  int32_t step, counter, flags, episode;
};

template <typename T>
struct Deriv { T vx, vy, vz, ax, ay, az, dqw, dqx, dqy, dqz, dwx, dwy, dwz; };

// All floating-point contraction is explicit: the library is compiled with -ffp-contract=off and every
// fused multiply-add below is written as fma_().  The step kernel, the rollout kernel and any future
// variant therefore produce bit-identical trajectories (tests/test_gpu_parity.py::test_rollout_*).
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T> __device__ __forceinline__ T dot3_(T a0, T a1, T a2, T b0, T b1, T b2) { return fma_(a0, b0, fma_(a1, b1, a2 * b2)); }

// ODE right-hand side (quadcopter.py:66-103).  F, M: post-mixer wrench, constant over the step.
template <typename T, typename PT>
__device__ __forceinline__ Deriv<T> rhs(const PT& P, T vx, T vy, T vz, T qw, T qx, T qy, T qz, T p, T q, T r, T Fm,
                                        T Mx, T My, T Mz) {
  Deriv<T> d;
  // third column of wRb for the NORMALISED quaternion: quadratic in q/|q| => divide by |q|^2 once
  const T n2 = fma_(qw, qw, fma_(qx, qx, fma_(qy, qy, qz * qz)));
  const T in2 = rcp_(n2);
  const T s = (Fm + Fm) * in2;                                   // 2 F / (m |q|^2)
  d.vx = vx; d.vy = vy; d.vz = vz;                               // :89-91
  d.ax = s * fma_(qx, qz, -(qw * qy));                           // :73-74
  d.ay = s * fma_(qy, qz, qw * qx);
  d.az = fma_(-s, fma_(qx, qx, qy * qy), Fm) - P.g;
  // qdot = -1/2 Omega(p,q,r) q + 2 (1-|q|^2) q                  :77-82
  const T k = fma_(T(-2), n2, T(2));
  d.dqw = fma_(T(0.5), fma_(p, qx, fma_(q, qy, r * qz)), k * qw);
  d.dqx = fma_(T(-0.5), fma_(p, qw, fma_(q, qz, -(r * qy))), k * qx);
  d.dqy = fma_(T(-0.5), fma_(q, qw, fma_(r, qx, -(p * qz))), k * qy);
  d.dqz = fma_(T(-0.5), fma_(r, qw, fma_(p, qy, -(q * qx))), k * qz);
  // pqrdot = invI (M - w x (I w))                               :86-87
  const T i0 = dot3_(P.Ixx, P.Ixy, P.Ixz, p, q, r);
  const T i1 = dot3_(P.Ixy, P.Iyy, P.Iyz, p, q, r);
  const T i2 = dot3_(P.Ixz, P.Iyz, P.Izz, p, q, r);
  const T t0 = Mx - fma_(q, i2, -(r * i1));
  const T t1 = My - fma_(r, i0, -(p * i2));
  const T t2 = Mz - fma_(p, i1, -(q * i0));
  d.dwx = dot3_(P.Jxx, P.Jxy, P.Jxz, t0, t1, t2);
  d.dwy = dot3_(P.Jxy, P.Jyy, P.Jyz, t0, t1, t2);
  d.dwz = dot3_(P.Jxz, P.Jyz, P.Jzz, t0, t1, t2);
  return d;
}

// ---- per-episode dynamics randomisation (include/amenv.h amenv_set_randomization) ------------------------------
// Ranges travel as a kernel argument of their own, in the DR instantiations only (HotParams is at its SGPR budget).  A factor is
// lo + span * u, span = hi - lo, all in fp32 (the library is built with -ffp-contract=off: a multiply, then an add).
struct DrRanges { float lo[3], span[3]; };   // [0] mass, [1] inertia, [2] thrust (one draw per rotor)
// ---- body-rate actions (include/amenv.h amenv_set_rate_control) ------------------------------------------------------
// The block travels behind the ranges, so every kernel built with kDynDr receives it: no switch bit and no instantiation of its own.
// on: 0 off, 1 the rate loop, 3 the rate loop with the gyroscopic feed-forward (wave-uniform: it sits in a scalar register).
struct RateBlock { int32_t on; float max_rate[3], gain[3], inv_ms; };   // rad/s, 1/s, float(1 / moment_scale) formed on the host in fp64
// ---- per-episode rotor failure (include/amenv.h amenv_set_rotor_failure) ----------------------------------------------
// The block travels behind the rate block, as that one behind the ranges: no switch bit and no instantiation of its own.  Five dwords, packed
// on the host, because every kernel that carries them is at its scalar-register budget:
//   ctl     0 = off (wave-uniform: a handle with randomisation but without the failure draws no second Philox block), else
//           bit 31 | count << 17 | p16, with p16 = floor(probability * 65536 + 0.5) in 0..65536 and count the number of admissible rotors;
//   rotors  the admissible rotors in ascending order, four bits each (entry k in bits 4 k ..): the k-th one is a shift and a mask on the
//           lane's k, where a walk over a bit mask cost seven pairs of scalar registers for its lane masks;
//   onset   lo | (hi - lo) << 16;   rem_lo, rem_span: the remaining fraction's lo and hi - lo, fp32.
struct FailBlock { uint32_t ctl, rotors, onset; float rem_lo, rem_span; };
static_assert(sizeof(DrRanges) == 24 && sizeof(RateBlock) == 32 && sizeof(FailBlock) == 20, "the blocks behind the ranges are packed dwords");
template <bool ON> struct DrArg { DrRanges r; RateBlock q; FailBlock x; };
static_assert(sizeof(DrArg<true>) == 76 && alignof(DrArg<true>) == 4, "ranges | rate block | failure block, no padding between them");
template <> struct DrArg<false> { int unused; };
// Per-lane factors of the lane's current episode, drawn once per launch (and again after an auto-reset inside a rollout); empty when off.
// F = sum s_r t_r and M = mixm (s . t); translational acceleration F / (km m); rotational J (M / kI - w x I w).
template <typename T, int NROT, bool ON> struct DynFac {};
template <typename T, int NROT> struct DynFac<T, NROT, true> {
  T s[NROT];        // thrust factor per rotor
  T inv_mass;       // 1 / (km m)
  T inv_ki;         // 1 / kI
};

// ---- first-order rotor lag (include/amenv.h amenv_set_rotor_lag) -------------------------------------------------
// One state number per env and rotor: w = sqrt(delivered thrust), rotor speed up to sqrt(k_f).  Once per control step the commanded
// speed c = sqrt(clamped thrust) is approached by w' = w + a (c - w), a = a_up when the rotor speeds up, else a_down; the rotor delivers
// w'^2 over the whole step.  The states live in a side buffer of the handle, tiled like the blob: [n_pad / 64][NROT][64] values of T (one
// coalesced load and store per lane and rotor, and ONE address per lane: the rotors are constant offsets from it -- with [NROT][n_pad] rows
// the closed-loop kernel kept NROT 64-bit addresses alive from its first load to its last store and spilled them), with the episode-start
// values w0[NROT] behind them (read on the reset path only); the buffer and the two coefficients
// travel in a kernel argument of their own, in the LAG instantiations only (HotParams is at its SGPR budget: the fp64 helper-wave kernel
// has no scalar register left for w0[]).  LAG is built only together with DR (unit ranges when randomisation is off).
template <typename T, int NROT, bool ON> struct LagArg { int unused; };
template <typename T, int NROT> struct LagArg<T, NROT, true> {
  T* w;              // [n_pad / 64][NROT][64] rotor states | [NROT] w0: rotors at the nominal hover command
  uint32_t n_pad;    // the handle's padded env count (whole tiles)
  T a_up, a_down;    // -expm1(-dt / tau), formed on the host in fp64
};
// ---- sensor noise on the observations (include/amenv.h amenv_set_sensor_noise) -----------------------------------
// Four standard deviations (position m, velocity m/s, body rate rad/s, attitude rad); they travel behind the lag's fields in the NOISE
// instantiations only.  NOISE is built only together with DR (unit ranges when randomisation is off), fp32 only.
struct NoiseSig { float p, v, w, a; };
template <bool ON> struct NoiseArg { static constexpr bool on = false; static constexpr int lds_ne = 0; };
template <> struct NoiseArg<true> {
  static constexpr bool on = true; static constexpr int lds_ne = 0;
  NoiseSig s;
  __device__ __forceinline__ float* column() const { return nullptr; }
};
// The closed-loop kernel's NORM forms have no VGPR to spare: there the perturbed copy goes through an LDS column of the lane's own,
// [13][NE] floats (no barrier): each Philox block's four results leave the registers before the next block is drawn, and observe() reads
// the copy back one number at a time.
template <int NE> struct NoiseLds {
  static constexpr bool on = true; static constexpr int lds_ne = NE;
  NoiseSig s; float* col;
  __device__ __forceinline__ float* column() const { return col; }
};
// ---- per-episode actuation latency (include/amenv.h amenv_set_action_delay) ---------------------------------------
// Each env applies the action row it was given d control steps ago, d drawn per episode from [lo, lo + span - 1].  The last 8 given rows
// live in a side buffer of the handle, tiled like the lag's: float4 [n_pad / 64][8 slots][64 envs] (a lane moves a whole row with one
// dword x4 access, a wave 1 KiB), and behind them one word per env, int32 [n_pad]: d | head << 4.  The ring is ordered by a head index of its
// own (the slot the next given row goes to), never by the env's step field: the row given k + 1 steps ago sits in slot (head - 1 - k) & 7.
// The fields travel behind the noise's in the DELAY instantiations only.  DELAY is built only together with DR, fp32 only.
template <bool ON> struct DelayArg { static constexpr bool on = false; };
template <> struct DelayArg<true> {
  static constexpr bool on = true;
  float4* h;           // [n_pad / 64][8][64] given rows | int32 [n_pad] d | head << 4
  uint32_t n_pad;      // the handle's padded env count (whole tiles)
  int32_t lo, span;    // min_steps, max_steps - min_steps + 1
  int32_t hist;        // action history: 0..2 given rows appended to every observation row; wave-uniform, in the struct's tail padding
};
struct DelayLane { int d, head; };
// The rows an observation row of the DELAY forms ends with: n of them (wave-uniform), g0 given in this step, g1 the step before.
struct HistRows {
  static constexpr bool on = true;
  int n; float4 g0, g1;
  __device__ __forceinline__ void hover() { g0 = g1 = make_float4(1.0f, 0.0f, 0.0f, 0.0f); }
};
struct NoHist { static constexpr bool on = false; };
// ---- the switch set ---------------------------------------------------------------------------------------------
// One template parameter names the opt-in features a kernel is built with: a mask of these bits.
constexpr unsigned kDynDr = 1, kDynLag = 2, kDynNoise = 4, kDynDelay = 8, kDynAll = 15;
// Not a switch: a FORM of a kernel, named on top of its switch set (template arguments 17u..31u; the kernel's argument stays the set's DynArg).
// The kernels that cannot carry the rotor failure's code without scratch or spilled registers -- the closed loop's NORM forms, the fp64 step
// kernels -- have instantiations of their own with it, which a handle runs only while the failure is set; their other forms hold none of its
// code and draw the randomisation as before it, so that a handle without the failure pays nothing.
constexpr unsigned kDynFailForm = 16;
// The build rule, stated once: LAG, NOISE and DELAY are built only together with DR (unit ranges when randomisation is off); NOISE and
// DELAY are fp32 only; every switch is built for rigid vehicles only.
template <typename T, int NJ> constexpr bool dyn_admitted(unsigned dyn) {
  return dyn <= kDynAll && (dyn == 0 || NJ == 0) && (!(dyn & (kDynLag | kDynNoise | kDynDelay)) || (dyn & kDynDr)) &&
         (!(dyn & (kDynNoise | kDynDelay)) || sizeof(T) == 4);
}
// The one kernel argument that carries the switches: the ranges (an unused word when DR is off: the kernels without switches keep their
// argument segment), behind them the lag's block, the noise's sigmas and the latency's fields, each only in the sets that have its bit.
// A part that is off is an empty base; a part that is on is a plain aggregate, so the next one starts behind its padded end.
template <bool ON> struct DynPartR { DrArg<ON> R; };
template <typename T, int NROT, bool ON> struct DynPartL {};
template <typename T, int NROT> struct DynPartL<T, NROT, true> { LagArg<T, NROT, true> L; };
template <bool ON> struct DynPartZ {};
template <> struct DynPartZ<true> { NoiseArg<true> Z; };
template <bool ON> struct DynPartD {};
template <> struct DynPartD<true> { DelayArg<true> D; };
template <typename T, int NROT, unsigned DYN>
struct DynArg : DynPartR<(DYN & kDynDr) != 0>, DynPartL<T, NROT, (DYN & kDynLag) != 0>, DynPartZ<(DYN & kDynNoise) != 0>, DynPartD<(DYN & kDynDelay) != 0> {};
template <typename T, int NROT, unsigned DYN>
__host__ __device__ __forceinline__ NoiseArg<(DYN & kDynNoise) != 0> noise_of(const DynArg<T, NROT, DYN>& a) {
  if constexpr ((DYN & kDynNoise) != 0) return a.Z; else return NoiseArg<false>{};
}
// The argument bytes are those of a struct with the parts that are on as plain members: each part at the next multiple of its alignment
// behind the part before it.  Size and alignment are pinned here; the offsets follow from the holders being plain aggregates, whose tail
// padding (LagArg<float>'s) the ABI gives to no later base -- the size alone would not tell where the alignment rounds it up anyway.
template <typename P> constexpr void dyn_member(bool on, size_t& end, size_t& align) {
  if (on) { end = (end + alignof(P) - 1) / alignof(P) * alignof(P) + sizeof(P); align = alignof(P) > align ? alignof(P) : align; }
}
template <typename T, int NROT, unsigned DYN = 0> constexpr bool dyn_layouts_ok() {   // DYN and every admitted set above it
  if constexpr (DYN > kDynAll) return true;
  else if constexpr (!dyn_admitted<T, 0>(DYN)) return dyn_layouts_ok<T, NROT, DYN + 1>();
  else {
    using A = DynArg<T, NROT, DYN>;
    size_t end = 0, align = 1;
    dyn_member<DrArg<(DYN & kDynDr) != 0>>(true, end, align);
    dyn_member<LagArg<T, NROT, true>>(DYN & kDynLag, end, align);
    dyn_member<NoiseArg<true>>(DYN & kDynNoise, end, align);
    dyn_member<DelayArg<true>>(DYN & kDynDelay, end, align);
    return sizeof(A) == (end + align - 1) / align * align && alignof(A) == align && std::is_trivially_copyable<A>::value && dyn_layouts_ok<T, NROT, DYN + 1>();
  }
}
static_assert(dyn_layouts_ok<float, 4>() && dyn_layouts_ok<float, 6>() && dyn_layouts_ok<double, 4>() && dyn_layouts_ok<double, 6>() && dyn_layouts_ok<float, AMENV_MAX_ROTORS>() &&
              dyn_layouts_ok<double, AMENV_MAX_ROTORS>(), "a DynArg has the size and alignment of its parts as plain members of one struct");
// env i's rotor r sits at lag_slot(i) + 64 r
template <int NROT> __device__ __forceinline__ size_t lag_slot(int i) { return size_t(i >> 6) * (NROT * 64) + size_t(i & 63); }
// What dynamics() filters through: get(r) / set(r, w') and the two coefficients.  LagLane keeps the rotor states in the lane's registers
// (empty when off); LagLds keeps them in an LDS column of the lane's own, [2 NROT + 2][NE] floats, for the closed-loop kernel whose NORM
// forms have no VGPR to spare: one rotor's state is in a register at a time, and the randomisation's per-lane factors (s_r, 1 / (km m),
// 1 / kI) sit in the same column instead of in DynFac's registers (holds_s), which is what makes the room.
template <typename T, int NROT, bool ON> struct LagLane { static constexpr bool on = false, holds_s = false; };
template <typename T, int NROT> struct LagLane<T, NROT, true> {
  static constexpr bool on = true, holds_s = false;
  T w[NROT]; T a_up, a_down;
  __device__ __forceinline__ T get(int r) const { return w[r]; }
  __device__ __forceinline__ void set(int r, T v) { w[r] = v; }
};
template <int NROT, int NE, bool ON> struct LagLds { static constexpr bool on = false, holds_s = false; };
template <int NROT, int NE> struct LagLds<NROT, NE, true> {
  static constexpr bool on = true, holds_s = true;
  float* col; float a_up, a_down;   // col: &wl[env within the workgroup]; rows 0..NROT-1 w_r, rows NROT.. s_r, then 1 / (km m), 1 / kI
  __device__ __forceinline__ float get(int r) const { return col[r * NE]; }
  __device__ __forceinline__ void set(int r, float v) { col[r * NE] = v; }
  __device__ __forceinline__ float s(int r) const { return col[(NROT + r) * NE]; }
  __device__ __forceinline__ float inv_mass() const { return col[2 * NROT * NE]; }
  __device__ __forceinline__ float inv_ki() const { return col[(2 * NROT + 1) * NE]; }
  __device__ __forceinline__ void put(const DynFac<float, NROT, true>& d) {
#pragma unroll
    for (int r = 0; r < NROT; r++) col[(NROT + r) * NE] = d.s[r];
    col[2 * NROT * NE] = d.inv_mass; col[(2 * NROT + 1) * NE] = d.inv_ki;
  }
};
template <typename T, int NROT>
__device__ __forceinline__ void lag_load(const LagArg<T, NROT, true>& L, int i, LagLane<T, NROT, true>& g) {
  g.a_up = L.a_up; g.a_down = L.a_down;
  const T* p = L.w + lag_slot<NROT>(i);
#pragma unroll
  for (int r = 0; r < NROT; r++) g.w[r] = p[r * 64];
}
template <typename T, int NROT>
__device__ __forceinline__ void lag_store(const LagArg<T, NROT, true>& L, int i, const LagLane<T, NROT, true>& g) {
  T* p = L.w + lag_slot<NROT>(i);
#pragma unroll
  for (int r = 0; r < NROT; r++) p[r * 64] = g.w[r];
}
template <typename T, int NROT>
__device__ __forceinline__ void lag_restart(const LagArg<T, NROT, true>& L, LagLane<T, NROT, true>& g) {   // a new episode starts
#pragma unroll
  for (int r = 0; r < NROT; r++) g.w[r] = L.w[size_t(NROT) * L.n_pad + r];
}

// Quadcopter.update (quadcopter.py:105-114) with RK4 in place of odeint.
template <typename T, int NROT, int KW, bool DR = false, typename LG = LagLane<T, NROT, false>>
__device__ __forceinline__ void dynamics(const HotParams<T, NROT>& P, Env<T, KW>& e, float a0, float a1, float a2, float a3,
                                         const DynFac<T, NROT, DR>& df = DynFac<T, NROT, DR>{}, LG* lg = nullptr) {
  // action scaling in fp32, left to right (rl_env_scaledObs.py:125-126)
  const float Ff = (a0 * P.mass_f) * P.g_f;
  const T u0 = T(Ff), u1 = T(a1 * P.mscale_f), u2 = T(a2 * P.mscale_f), u3 = T(a3 * P.mscale_f);
  // mixer -> per-rotor clamp -> re-mix (:109-112)
  T F = T(0), Mx = T(0), My = T(0), Mz = T(0);
#pragma unroll
  for (int r = 0; r < NROT; r++) {
    if (NROT == AMENV_MAX_ROTORS && r >= P.n_rotors) break;  // generic instantiation: runtime rotor count
    T t = fma_(P.alloc[r][0], u0, fma_(P.alloc[r][1], u1, fma_(P.alloc[r][2], u2, P.alloc[r][3] * u3)));
    t = clamp_(t, P.tmin[r], P.tmax[r]);   // np.maximum(np.minimum(t, max), min), quadcopter.py:110
    if constexpr (LG::on) {                // the rotor's speed follows the command's with a first-order lag; it delivers w'^2
      const T c = sqrt_(t);
      const T w = lg->get(r);
      const T wn = fma_(c > w ? lg->a_up : lg->a_down, c - w, w);
      lg->set(r, wn);
      t = wn * wn;
    }
    if constexpr (DR) {                    // the rotor delivers s_r of its (nominally saturated) command
      if constexpr (LG::holds_s) t = t * lg->s(r); else t = t * df.s[r];
    }
    F = F + t; Mx = fma_(P.mixm[0][r], t, Mx); My = fma_(P.mixm[1][r], t, My); Mz = fma_(P.mixm[2][r], t, Mz);
  }
  T Fm;
  if constexpr (DR && LG::holds_s) { const T ik = lg->inv_ki(); Fm = F * lg->inv_mass(); Mx = Mx * ik; My = My * ik; Mz = Mz * ik; }
  else if constexpr (DR) { Fm = F * df.inv_mass; Mx = Mx * df.inv_ki; My = My * df.inv_ki; Mz = Mz * df.inv_ki; }
  else Fm = F * P.inv_mass;
  const T h = P.h, hh = T(0.5) * h, h6 = h * T(1.0 / 6.0);
  int it = 0;
  do {  // substeps >= 1 (validated at create): no loop guard in front of the first stage
    const Deriv<T> k1 = rhs<T>(P, e.vx, e.vy, e.vz, e.qw, e.qx, e.qy, e.qz, e.wx, e.wy, e.wz, Fm, Mx, My, Mz);
    const Deriv<T> k2 = rhs<T>(P, fma_(hh, k1.ax, e.vx), fma_(hh, k1.ay, e.vy), fma_(hh, k1.az, e.vz), fma_(hh, k1.dqw, e.qw),
                            fma_(hh, k1.dqx, e.qx), fma_(hh, k1.dqy, e.qy), fma_(hh, k1.dqz, e.qz), fma_(hh, k1.dwx, e.wx),
                            fma_(hh, k1.dwy, e.wy), fma_(hh, k1.dwz, e.wz), Fm, Mx, My, Mz);
    const Deriv<T> k3 = rhs<T>(P, fma_(hh, k2.ax, e.vx), fma_(hh, k2.ay, e.vy), fma_(hh, k2.az, e.vz), fma_(hh, k2.dqw, e.qw),
                            fma_(hh, k2.dqx, e.qx), fma_(hh, k2.dqy, e.qy), fma_(hh, k2.dqz, e.qz), fma_(hh, k2.dwx, e.wx),
                            fma_(hh, k2.dwy, e.wy), fma_(hh, k2.dwz, e.wz), Fm, Mx, My, Mz);
    const Deriv<T> k4 = rhs<T>(P, fma_(h, k3.ax, e.vx), fma_(h, k3.ay, e.vy), fma_(h, k3.az, e.vz), fma_(h, k3.dqw, e.qw),
                            fma_(h, k3.dqx, e.qx), fma_(h, k3.dqy, e.qy), fma_(h, k3.dqz, e.qz), fma_(h, k3.dwx, e.wx),
                            fma_(h, k3.dwy, e.wy), fma_(h, k3.dwz, e.wz), Fm, Mx, My, Mz);
    // y += h/6 (k1 + 2 k2 + 2 k3 + k4)
#define AMENV_RK4(x, f) e.x = fma_(h6, fma_(T(2), k2.f + k3.f, k1.f + k4.f), e.x)
    AMENV_RK4(px, vx); AMENV_RK4(py, vy); AMENV_RK4(pz, vz);
    AMENV_RK4(vx, ax); AMENV_RK4(vy, ay); AMENV_RK4(vz, az);
    AMENV_RK4(qw, dqw); AMENV_RK4(qx, dqx); AMENV_RK4(qy, dqy); AMENV_RK4(qz, dqz);
    AMENV_RK4(wx, dwx); AMENV_RK4(wy, dwy); AMENV_RK4(wz, dwz);
#undef AMENV_RK4
  } while (++it < P.substeps);
  const T rn = rsqrt_(fma_(e.qw, e.qw, fma_(e.qx, e.qx, fma_(e.qy, e.qy, e.qz * e.qz))));   // :114
  e.qw *= rn; e.qx *= rn; e.qy *= rn; e.qz *= rn;
}

template <typename T, int KW>
__device__ __forceinline__ void current_waypoint(int K, const Env<T, KW>& e, int idx, T& cx, T& cy, T& cz) {
  cx = e.wp[0][0]; cy = e.wp[0][1]; cz = e.wp[0][2];
#pragma unroll
  for (int k = 1; k < KW; k++)
    if (k < K && idx >= k) { cx = e.wp[k][0]; cy = e.wp[k][1]; cz = e.wp[k][2]; }
}

// The point the waypoint task measures from: the base position (the reference), or with EE the arm's tool point.
template <bool EE, typename T, int KW>
__device__ __forceinline__ void task_point(const Env<T, KW>& e, bool ee_task, T& tx, T& ty, T& tz) {
  tx = e.px; ty = e.py; tz = e.pz;
  if constexpr (EE) {
    if (ee_task) { tx = e.px + e.eox; ty = e.py + e.eoy; tz = e.pz + e.eoz; }
  }
}

// _get_observation (rl_env_scaledObs.py:98-121)
template <typename T, int KW, bool EE = false>
__device__ __forceinline__ void observe(int K, const Env<T, KW>& e, float* o, bool ee_task = false) {
  const int idx = e.flags & 15;
  T cx, cy, cz;
  current_waypoint(K, e, idx, cx, cy, cz);
  T tx, ty, tz;
  task_point<EE>(e, ee_task, tx, ty, tz);
  // scalings as multiplications by the rounded reciprocal (<= 1 ulp from the reference's divisions)
  const T c10 = T(0.1), c5 = T(0.2), c2 = T(0.5);
  o[0] = float(e.px * c10); o[1] = float(e.py * c10); o[2] = float(e.pz * c10);
  o[3] = float(e.vx * c5); o[4] = float(e.vy * c5); o[5] = float(e.vz * c5);
  o[6] = float(e.qw); o[7] = float(e.qx); o[8] = float(e.qy); o[9] = float(e.qz);
  o[10] = float(e.wx * c5); o[11] = float(e.wy * c5); o[12] = float(e.wz * c5);
  o[13] = float((cx - tx) * c2); o[14] = float((cy - ty) * c2); o[15] = float((cz - tz) * c2);
  T nx = T(0), ny = T(0), nz = T(0);
#pragma unroll
  for (int k = 1; k < KW; k++)
    if (k < K && idx == k - 1) { nx = e.wp[k][0] - cx; ny = e.wp[k][1] - cy; nz = e.wp[k][2] - cz; }
  o[16] = float(nx * c2); o[17] = float(ny * c2); o[18] = float(nz * c2);
  o[19] = float(e.final_yaw * T(0.31830988618379067154));
}

// One WaypointQuadEnv.step (rl_env_scaledObs.py:123-196) after the dynamics update.
// Returns info bits; reward in `reward`.  Mutates the episode registers.
// act_nf(): the summed nonfinite_mark of the action row the step applied; called inside the guard's branch only, so that a handle without
// AMENV_FLAG_NAN_GUARD runs none of it.
template <typename T, int KW, bool EE = false, typename PT, typename AF = NoActionMark<T>>
__device__ __forceinline__ uint32_t task_step(const PT& P, Env<T, KW>& e, T& reward, const AF& act_nf = AF{}) {
  const int K = KW == 1 ? 1 : P.K;
  uint32_t bits = 0;
  int idx = e.flags & 15;
  bool fwr = (e.flags & AMENV_FLAGBIT_FWR) != 0;
  bool cact = (e.flags & AMENV_FLAGBIT_COUNTER_ACTIVE) != 0;
  const bool truncated = e.step >= P.max_steps;                         // :144
  e.step += 1;                                                          // :145
  if (truncated) bits |= AMENV_INFO_TRUNCATED;

  // (the oracle tests the joint angles and rates too; they are not summed here: a non-finite one reaches the base rows within the step it
  // is integrated in -- tests/test_gpu_flag_sweep.py puts NaN, +Inf and -Inf into each of them on every arm kernel)
  if (P.flags & AMENV_FLAG_NAN_GUARD) {                                 // deviation, see DESIGN.md
    const T sum = e.px + e.py + e.pz + e.vx + e.vy + e.vz + e.qw + e.qx + e.qy + e.qz + e.wx + e.wy + e.wz + act_nf();
    if (!finite_(sum)) { reward = T(-100); return bits | AMENV_INFO_TERMINATED | AMENV_INFO_NONFINITE; }
  }
  T cx, cy, cz;
  current_waypoint(K, e, idx, cx, cy, cz);
  // ---- _calculate_reward (:198-231)
  T tx, ty, tz;
  task_point<EE>(e, P.ee_task != 0, tx, ty, tz);
  const T dx = tx - cx, dy = ty - cy, dz = tz - cz;
  const T dist = sqrt_(dot3_(dx, dy, dz, dx, dy, dz));                    // :204
  T r_dist = T(-10) * dist;                                             // :207
  const T v2 = dot3_(e.vx, e.vy, e.vz, e.vx, e.vy, e.vz);
  const T w2 = dot3_(e.wx, e.wy, e.wz, e.wx, e.wy, e.wz);
  const T vn = sqrt_(v2), wn = sqrt_(w2);
  T r_speed = T(-0.1) * v2;                                             // :208
  if (wn > T(0.1)) r_speed -= T(0.01) * w2;                             // :209-210
  T r_time = T(-0.1);                                                   // :211
  T r_prog = T(0);
  if (e.last_distance >= T(0)) {                                        // :214-220
    r_prog = T(20) * (e.last_distance - dist);
    if (r_prog > T(0)) r_prog += T(2);
  }
  e.last_distance = dist;                                               // :222
  if (fwr) {                                                            // :224-228
    r_prog = T(0); r_time = T(0);
    if (dist < T(0.1)) r_dist = T(1);
  }
  reward = ((r_dist + r_speed) + r_time) + r_prog;                      // :231

  bool returned = false;
  if (dist < T(0.1)) {                                                  // :147
    if (!fwr) { idx += 1; reward += T(100); }                           // :148-150
    if (idx >= K) {                                                     // :153 (else: next waypoint, fall through)
      idx = K;                                                          // waypoint_index == len(list)
      // roll, pitch, yaw (utils2/utils.py:4-9 closed form); only the hold-phase bonuses use them
      const T roll = atan2_(T(2) * fma_(e.qw, e.qx, e.qy * e.qz), fma_(T(-2), fma_(e.qx, e.qx, e.qy * e.qy), T(1)));
      T sp = T(2) * fma_(e.qw, e.qy, -(e.qz * e.qx));
      sp = sp > T(1) ? T(1) : (sp < T(-1) ? T(-1) : sp);
      const T pitch = asin_(sp);
      const T yaw = atan2_(T(2) * fma_(e.qw, e.qz, e.qx * e.qy), fma_(T(-2), fma_(e.qy, e.qy, e.qz * e.qz), T(1)));
      // bonuses: divisions by constants as multiplications by the rounded reciprocal (<= 1 ulp), selects not branches
      const T two_pi = T(6.28318530717958647692), inv_two_pi = T(0.15915494309189533577);
      const T dyaw = abs_(yaw - e.final_yaw);
      const T yaw_f = dyaw < two_pi ? T(1) - dyaw * inv_two_pi : T(0);     // (1 - |dyaw|/2pi) or 0   :163,169
      bits |= AMENV_INFO_SUCCESS;
      if (vn < T(0.1) && wn < T(0.1)) bits |= AMENV_INFO_STOPPED;
      const T ar = abs_(roll), ap = abs_(pitch);
      const T roll_b = ar < T(0.2) ? T(10) * (T(1) - ar * T(5)) : T(-0.1) * ar;      // :170,176
      const T pitch_b = ap < T(0.2) ? T(10) * (T(1) - ap * T(5)) : T(-0.1) * ap;     // :171,177
      const T stop_b = vn < T(1) ? T(150) * (T(1) - v2) : T(0);                      // :162
      const T r_first = ((reward + T(200)) + stop_b) + T(100) * yaw_f;               // :164 first arrival
      const T r_hold = ((reward + T(30) * yaw_f) + roll_b) + pitch_b;                // :173,179 holding
      reward = fwr ? r_hold : r_first;
      if (fwr) {                                                        // :165-179 holding
        if (e.counter <= P.counter_limit) e.counter += 1;               // :166-167
        else bits |= AMENV_INFO_TERMINATED;                             // :174-179
      }
      cact = true; fwr = true;                                          // :157-158 (no-ops when already holding)
      returned = true;
    }
  }
  if (!returned) {
    if (cact) e.counter += 1;                                           // :181-182
    if (e.pz < T(0.1)) {                                                // :188-192
      reward -= T(100);
      if (e.vz < T(0)) reward += e.vz * T(100);
      bits |= AMENV_INFO_TERMINATED | AMENV_INFO_CRASHED;
    } else if (sqrt_(dot3_(e.px, e.py, e.pz, e.px, e.py, e.pz)) > T(10)) { // :193-195
      reward -= T(100);
      bits |= AMENV_INFO_TERMINATED | AMENV_INFO_OOB;
    }
  }
  e.flags = (idx & 15) | (fwr ? AMENV_FLAGBIT_FWR : 0) | (cact ? AMENV_FLAGBIT_COUNTER_ACTIVE : 0);
  return bits;
}

__device__ __forceinline__ float u01(uint32_t r) { return float(r >> 8) * 5.9604644775390625e-08f; }   // [0,1), 24 bits, exact

// ---- v1 task (v1/rl_env_scaledObs.py, v1/rl_env.py): 17-D observation, per-episode waypoint count in flags bits 4-7 ----
template <typename T, int KW>
__device__ __forceinline__ void observe_v1(bool raw, const Env<T, KW>& e, float* o) {        // :65-83
  const int idx = e.flags & 15, K = (e.flags >> 4) & 15;
  T cx, cy, cz;
  current_waypoint(K, e, idx, cx, cy, cz);
  const T c10 = raw ? T(1) : T(0.1), c5 = raw ? T(1) : T(0.2), c2 = raw ? T(1) : T(0.5);
  o[0] = float(e.px * c10); o[1] = float(e.py * c10); o[2] = float(e.pz * c10);
  o[3] = float(e.vx * c5); o[4] = float(e.vy * c5); o[5] = float(e.vz * c5);
  o[6] = float(e.qw); o[7] = float(e.qx); o[8] = float(e.qy); o[9] = float(e.qz);
  o[10] = float(e.wx * c5); o[11] = float(e.wy * c5); o[12] = float(e.wz * c5);
  o[13] = float((cx - e.px) * c2); o[14] = float((cy - e.py) * c2); o[15] = float((cz - e.pz) * c2);
  o[16] = idx >= K - 1 ? 1.0f : 0.0f;                                                         // :80 is_final
}

// One v1 step after the dynamics update: v1/rl_env_scaledObs.py:93-140 (+ _calculate_reward :142-168).
template <typename T, int KW, typename PT, typename AF = NoActionMark<T>>
__device__ __forceinline__ uint32_t task_step_v1(const PT& P, Env<T, KW>& e, T& reward, const AF& act_nf = AF{}) {
  uint32_t bits = 0;
  int idx = e.flags & 15;
  const int K = (e.flags >> 4) & 15;
  if (P.flags & AMENV_FLAG_NAN_GUARD) {
    const T sum = e.px + e.py + e.pz + e.vx + e.vy + e.vz + e.qw + e.qx + e.qy + e.qz + e.wx + e.wy + e.wz + act_nf();
    if (!finite_(sum)) {
      if (e.step >= P.max_steps) bits |= AMENV_INFO_TRUNCATED;
      e.step += 1; reward = T(-100);
      return bits | AMENV_INFO_TERMINATED | AMENV_INFO_NONFINITE;
    }
  }
  T cx, cy, cz;
  current_waypoint(K, e, idx, cx, cy, cz);
  const T dx = e.px - cx, dy = e.py - cy, dz = e.pz - cz;
  const T dist = sqrt_(dot3_(dx, dy, dz, dx, dy, dz));                  // :148
  const T v2 = dot3_(e.vx, e.vy, e.vz, e.vx, e.vy, e.vz);
  const T w2 = dot3_(e.wx, e.wy, e.wz, e.wx, e.wy, e.wz);
  const T vn = sqrt_(v2), wn = sqrt_(w2);
  T r_speed = T(-0.1) * v2;                                             // :152
  if (wn > T(0.1)) r_speed -= T(0.01) * w2;                             // :153-154
  T r_prog = T(0);
  if (e.last_distance >= T(0)) {                                        // :158-164
    r_prog = T(20) * (e.last_distance - dist);
    if (r_prog > T(0)) r_prog += T(2);
  }
  e.last_distance = dist;                                               // :166
  reward = ((T(-2) * dist + r_speed) + T(-0.1)) + r_prog;               // :151,155,168
  // approach shaping: velocity component toward the waypoint (:102-110); dist == 0 -> NaN -> neither branch
  const T vtw = -dot3_(e.vx, e.vy, e.vz, dx, dy, dz) * rcp_(dist);
  if (dist < T(0.5)) {
    if (vtw > T(0.1)) reward += T(10);
    else if (vtw < T(0.1)) reward -= T(10);
  }
  bool final_reach = false;
  if (dist < T(0.1)) {                                                  // :111-124
    reward += T(100); idx += 1;
    if (idx >= K) {
      const T rot_b = wn < T(0.1) ? T(100) : T(-20) * wn;               // :122
      const T stop_b = vn < T(0.1) ? T(100) : T(-10) * vn;              // :123
      reward = ((reward + T(400)) + stop_b) + rot_b;                    // :124: returns BEFORE current_step += 1, truncated False
      bits = AMENV_INFO_TERMINATED | AMENV_INFO_SUCCESS | (vn < T(0.1) ? AMENV_INFO_STOPPED : 0u);
      final_reach = true;
    }
  }
  if (!final_reach) {
    if (e.step >= P.max_steps) bits |= AMENV_INFO_TRUNCATED;           // :126
    e.step += 1;                                                        // :127
    if (e.pz < T(0.1)) {                                                // :131-136
      reward -= T(100);
      if (e.vz < T(0)) reward += e.vz * T(100);
      bits |= AMENV_INFO_TERMINATED | AMENV_INFO_CRASHED;
    } else if (sqrt_(dot3_(e.px, e.py, e.pz, e.px, e.py, e.pz)) > T(10)) {  // :137-139
      reward -= T(100);
      bits |= AMENV_INFO_TERMINATED | AMENV_INFO_OOB;
    }
  }
  e.flags = (idx & 15) | (K << 4);
  return bits;
}

// v1 reset (v1/rl_env_scaledObs.py:32-63) from the 12 Philox words; DESIGN.md draw table "v1".
template <typename T, int KW>
__device__ __forceinline__ void reset_from_words_v1(int Kmax, Env<T, KW>& e, const uint32_t* r) {
  int K = 1 + int(r[2] >> 31);                                          // :38 randint(1,3)
  K = K < Kmax ? K : Kmax;
  e.px = T(fmaf(2.0f, u01(r[0]), -1.0f)); e.py = T(fmaf(2.0f, u01(r[1]), -1.0f)); e.pz = T(fmaf(1.0f, u01(r[3]), 1.0f));  // :36-37
  e.vx = e.vy = e.vz = T(0);
  e.qw = T(1); e.qx = e.qy = e.qz = T(0);
  e.wx = e.wy = e.wz = T(0);
#pragma unroll
  for (int k = 0; k < KW; k++) {
    const bool on = k < K && k < 2;
    const int b = 4 + 3 * (k < 2 ? k : 0);
    e.wp[k][0] = on ? T(fmaf(2.0f, u01(r[b]), -1.0f)) : T(0);          // :53-63
    e.wp[k][1] = on ? T(fmaf(2.0f, u01(r[b + 1]), -1.0f)) : T(0);
    e.wp[k][2] = on ? T(fmaf(2.0f, u01(r[b + 2]), 1.0f)) : T(0);
  }
  e.final_yaw = T(0); e.last_distance = T(-1); e.ep_return = T(0);
#pragma unroll
  for (int k = 0; k < AMENV_MAX_JOINTS; k++) { e.th[k] = T(0); e.thd[k] = T(0); }
  e.step = 0; e.counter = 0; e.flags = K << 4;
  e.episode += 1;
}

// ---- counter-based reset RNG: Philox4x32-10, key = seed, counter = (global env id, episode, block)
__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;  // one v_mad_u64_u32 each
    const uint32_t h0 = uint32_t(p0 >> 32), l0 = uint32_t(p0), h1 = uint32_t(p1 >> 32), l1 = uint32_t(p1);
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}


// The dynamics factors of (env, episode): ONE Philox block, counter (gid, episode, kDrBlock) -- a block index no other draw uses (resets
// 0..2, the quad / team / stage-wave kernels up to 4) -- cut into eight 16-bit uniforms u = w16 * 2^-16: u0 -> km, u1 -> kI, u2.. -> s_r.
// A pure function of (seed, gid, episode, ranges): no state is stored, a change of ranges applies from the next launch.
constexpr uint32_t kDrBlock = 0x44520000u;
template <int NROT>
__device__ __forceinline__ void dr_draw_keyed(uint32_t k0, uint32_t k1, const DrRanges& R, int64_t gid, int32_t episode, float* f /*[2 + NROT]*/) {
  static_assert(NROT <= 6, "eight 16-bit uniforms per block: km, kI and up to six rotors");
  uint32_t w[4];
  philox4x32_10(k0, k1, uint32_t(uint64_t(gid)), uint32_t(uint64_t(gid) >> 32), uint32_t(episode), kDrBlock, w);
#pragma unroll
  for (int k = 0; k < 2 + NROT; k++) {
    const uint32_t v = (k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu);
    const int q = k < 2 ? k : 2;
    f[k] = R.lo[q] + R.span[q] * (float(v) * 1.52587890625e-05f);
  }
}
template <int NROT>
__device__ __forceinline__ void dr_draw(const ColdParams& C, const DrRanges& R, int64_t gid, int32_t episode, float* f /*[2 + NROT]*/) {
  dr_draw_keyed<NROT>(C.seed_lo, C.seed_hi, R, gid, episode, f);
}
// The key of a draw inside a step or rollout kernel goes through an empty asm.  Every Philox block of a kernel has the same key, and the
// compiler would otherwise form the ten rounds' key words once, for this block, and keep all twenty alive for the reset path's blocks at the
// kernel's far end -- in kernels that have no scalar register to spare, where they end up spilled to vector lanes.  Two scalar
// adds per round buy them back.  (Read off the assembly of AMD clang 22.0.0git, ROCm 7.2.0, for gfx950: the values do not depend on it, the
// register numbers may.  To re-check after a compiler change: build.dump_asm() of this tree and of one without the asm, then
// tools/asm_kernel_diff.py A B --brief, and compare sgpr_spill_count of the step kernels.)
__device__ __forceinline__ void philox_own_key(const ColdParams& C, uint32_t& k0, uint32_t& k1) {
  k0 = C.seed_lo; k1 = C.seed_hi;
  asm volatile("" : "+s"(k0), "+s"(k1));
}
// OWN_KEY = false: the forms without the rotor failure's code of the kernels that have forms of their own with it (kDynFailForm).
template <typename T, int NROT, bool OWN_KEY = true>
__device__ __forceinline__ DynFac<T, NROT, true> dr_factors(const HotParams<T, NROT>& P, const ColdParams& C, const DrRanges& R, int64_t gid, int32_t episode) {
  float f[2 + NROT];
  uint32_t k0 = C.seed_lo, k1 = C.seed_hi;
  if constexpr (OWN_KEY) philox_own_key(C, k0, k1);
  dr_draw_keyed<NROT>(k0, k1, R, gid, episode, f);
  DynFac<T, NROT, true> d;
#pragma unroll
  for (int r = 0; r < NROT; r++) d.s[r] = T(f[2 + r]);
  d.inv_mass = P.inv_mass * rcp_(T(f[0]));
  d.inv_ki = rcp_(T(f[1]));
  return d;
}

// ---- rotor failure: the plan of (env, episode) and its effect on the thrust factors ------------------------------------------
// ONE Philox block, counter (gid, episode, kFailBlock); the top byte 0x46 is no other draw's (resets 0..4, randomisation 0x4452...., latency
// 0x4C54...., noise 0x4E......).  The 16-bit halves v0..v3 are cut as dr_draw cuts them.  v0 < p16: the episode has a failure (an integer
// compare: p16 = 0 never, p16 = 65536 always); v1 picks the k-th admissible rotor in ascending order, k = (v1 count) >> 16; v2 the onset step,
// lo + ((v2 span) >> 16) with span = hi - lo + 1 <= 65536 (the product fits 32 bits); v3 the remaining fraction lo + span * (v3 2^-16) in fp32,
// a multiply, then an add (dr_draw's arithmetic).  A pure function of (seed, gid, episode, block): no state is stored.
constexpr uint32_t kFailBlock = 0x46410000u;
// What a lane keeps of its plan: key = rotor << 16 | onset, or -1 (no failure in this episode, or the factor already holds it), and f.
struct FailLane { int32_t key; float f; };
template <int NROT>
__device__ __forceinline__ FailLane fail_draw(const ColdParams& C, const FailBlock& X, int64_t gid, int32_t episode) {
  uint32_t w[4];
  uint32_t k0 = C.seed_lo, k1 = C.seed_hi;
  asm volatile("" : "+v"(k0), "+v"(k1));   // a key of its own, as dr_factors', and in vector registers: the block sits behind a branch that costs the kernels no scalar register
  philox4x32_10(k0, k1, uint32_t(uint64_t(gid)), uint32_t(uint64_t(gid) >> 32), uint32_t(episode), kFailBlock, w);
  const uint32_t v0 = w[0] & 0xffffu, v1 = w[0] >> 16, v2 = w[1] & 0xffffu, v3 = w[1] >> 16;
  const uint32_t p16 = X.ctl & 0x1ffffu, count = (X.ctl >> 17) & 7u;
  const uint32_t rot = (X.rotors >> (((v1 * count) >> 16) << 2)) & 7u;
  const uint32_t onset = (X.onset & 0xffffu) + ((v2 * ((X.onset >> 16) + 1u)) >> 16);
  FailLane fl;
  fl.key = v0 < p16 ? int((rot << 16) | onset) : -1;
  fl.f = X.rem_lo + X.rem_span * (float(v3) * 1.52587890625e-05f);
  return fl;
}
// From the control step whose loaded step field reaches the onset, the failed rotor delivers f of what it delivered: s'_r = s_r * T(f), ONE
// rounded multiply, applied in place once; the key is spent with it.  A step kernel draws and tests once per launch; a rollout kernel draws at
// entry and after an auto-reset and tests in front of every step, so both compare the same step field with >=.
template <typename T, int NROT>
__device__ __forceinline__ void fail_hit(FailLane& fl, int32_t step, T* s) {
  if (fl.key >= 0 && step >= (fl.key & 0xffff)) {
    const int rot = fl.key >> 16;
    const T f = T(fl.f);
#pragma unroll
    for (int r = 0; r < NROT; r++) s[r] = r == rot ? s[r] * f : s[r];
    fl.key = -1;
  }
}
// The closed-loop kernel's NORM forms have no VGPR to spare: there the plan waits in an LDS column of the lane's own, [2][NE]
// words (key, f; no barrier), and a step reads the key alone.  s: the factors in registers, or null where they sit in the LagLds column
// `scol` (rows NROT.. hold s_r).
template <int NE> __device__ __forceinline__ void fail_put(int32_t* col, const FailLane& fl) { col[0] = fl.key; col[NE] = __float_as_int(fl.f); }
template <int NROT, int NE>
__device__ __forceinline__ void fail_hit_lds(int32_t* col, int32_t step, float* s, float* scol) {
  const int32_t key = col[0];
  if (key >= 0 && step >= (key & 0xffff)) {
    FailLane fl{key, __int_as_float(col[NE])};
    if (s) fail_hit<float, NROT>(fl, step, s);
    else { float* p = scol + (NROT + (key >> 16)) * NE; *p = *p * fl.f; }
    col[0] = -1;
  }
}
// the same for a plan in registers and factors in the LagLds column
template <int NROT, int NE>
__device__ __forceinline__ void fail_hit_scol(FailLane& fl, int32_t step, float* scol) {
  if (fl.key >= 0 && step >= (fl.key & 0xffff)) {
    float* p = scol + (NROT + (fl.key >> 16)) * NE;
    *p = *p * fl.f;
    fl.key = -1;
  }
}
// The step kernels' call, behind dr_factors: everything sits behind the wave-uniform flag.
template <typename T, int NROT>
__device__ __forceinline__ void fail_step(const ColdParams& C, const FailBlock& X, int64_t gid, int32_t episode, int32_t step, DynFac<T, NROT, true>& df) {
  if (X.ctl != 0u) {
    FailLane fl = fail_draw<NROT>(C, X, gid, episode);
    fail_hit<T, NROT>(fl, step, df.s);
  }
}

// ---- body-rate actions: the inner rate loop ---------------------------------------------------------------------------
// Entries 1..3 of the row the step is about to consume are body-rate commands; they become the equivalent moment action
//   w_cmd = a * max_rate;  u = gain * (w_cmd - w);  tau = I u (+ w x (I w));  a' = tau * (1 / moment_scale)
// with I the NOMINAL inertia (a flight controller does not know the episode's factor) and w the rates at the start of the step.  fp32, every
// operation named and in a fixed order, so that every kernel that inlines this forms the same bits (tests/rate_ref.py mirrors the order;
// the longest path has 8 roundings: w_cmd, the difference, u, the three of the I u row, the feed-forward's sum, the scaling).
template <typename PT>
__device__ __forceinline__ void rate_to_moment(const PT& P, const RateBlock& Q, float wx, float wy, float wz, float* act) {
  const float Ixx = float(P.Ixx), Ixy = float(P.Ixy), Ixz = float(P.Ixz), Iyy = float(P.Iyy), Iyz = float(P.Iyz), Izz = float(P.Izz);
  const float ux = __fmul_rn(Q.gain[0], __fadd_rn(__fmul_rn(act[1], Q.max_rate[0]), -wx));
  const float uy = __fmul_rn(Q.gain[1], __fadd_rn(__fmul_rn(act[2], Q.max_rate[1]), -wy));
  const float uz = __fmul_rn(Q.gain[2], __fadd_rn(__fmul_rn(act[3], Q.max_rate[2]), -wz));
  float tx = fmaf(Ixx, ux, fmaf(Ixy, uy, __fmul_rn(Ixz, uz)));
  float ty = fmaf(Ixy, ux, fmaf(Iyy, uy, __fmul_rn(Iyz, uz)));
  float tz = fmaf(Ixz, ux, fmaf(Iyz, uy, __fmul_rn(Izz, uz)));
  if (Q.on & 2) {   // + w x (I w): the term the rigid body's own right-hand side subtracts
    const float i0 = fmaf(Ixx, wx, fmaf(Ixy, wy, __fmul_rn(Ixz, wz)));
    const float i1 = fmaf(Ixy, wx, fmaf(Iyy, wy, __fmul_rn(Iyz, wz)));
    const float i2 = fmaf(Ixz, wx, fmaf(Iyz, wy, __fmul_rn(Izz, wz)));
    tx = __fadd_rn(tx, fmaf(wy, i2, -__fmul_rn(wz, i1)));
    ty = __fadd_rn(ty, fmaf(wz, i0, -__fmul_rn(wx, i2)));
    tz = __fadd_rn(tz, fmaf(wx, i1, -__fmul_rn(wy, i0)));
  }
  act[1] = __fmul_rn(tx, Q.inv_ms); act[2] = __fmul_rn(ty, Q.inv_ms); act[3] = __fmul_rn(tz, Q.inv_ms);
}
// The call of the kernels built with kDynDr: behind the action load and delay_apply, in front of the step.  A wave-uniform branch on the flag;
// the fp64 builds (logic gates of the dynamics, which no rate-mode handle runs) hold no rate code.
template <typename T, int KW, typename PT>
__device__ __forceinline__ void rate_apply(const PT& P, const RateBlock& Q, const Env<T, KW>& e, float* act) {
  if constexpr (sizeof(T) == 4) {
    if (Q.on != 0) rate_to_moment(P, Q, e.wx, e.wy, e.wz, act);
  }
}

// ---- sensor noise -----------------------------------------------------------------------------------------------
// Twelve unit samples per (seed, global env id, episode, step): three Philox blocks, counter (gid, episode, kNoiseTag | step << 2 | b); the
// top byte differs from every other draw's last counter word (resets 0..4, randomisation 0x4452....).  Word k of block b is sample 4 b + k:
// the sum of the word's four bytes (ONE v_sad_u8), centred and scaled -- an Irwin-Hall sum of four byte-uniforms, variance 21845, |n| <=
// 3.4506.  Integer arithmetic, one exact subtraction and one multiply: numpy reproduces it bit for bit (tests/noise_ref.py).
constexpr uint32_t kNoiseTag = 0x4E000000u;
constexpr float kNoiseScale = 0.006765875f;   // fp32 nearest to 21845^-1/2
__device__ __forceinline__ float noise_unit(uint32_t w) { return (float(int32_t(__builtin_amdgcn_sad_u8(w, 0u, 0u))) - 510.0f) * kNoiseScale; }
__device__ __forceinline__ void noise_block(uint32_t seed_lo, uint32_t seed_hi, int64_t gid, int32_t episode, int32_t step, uint32_t b, float* n /*[4]*/) {
  uint32_t w[4];
  philox4x32_10(seed_lo, seed_hi, uint32_t(uint64_t(gid)), uint32_t(uint64_t(gid) >> 32), uint32_t(episode),
                kNoiseTag | ((uint32_t(step) & 0x3FFFFFu) << 2) | b, w);
#pragma unroll
  for (int k = 0; k < 4; k++) n[k] = noise_unit(w[k]);
}
// Perturb a COPY of the state (the 13 numbers the observation reads) in place; the key's step is the env's step field as stored after the
// observation's step (0 for a post-reset row).  Samples 0..2 position, 3..5 velocity, 6..8 body rate: one fma each; 9..11 a small rotation
// d = sigma_a / 2 * n applied on the body side, q~ = q (x) (1, d) (Hamilton, scalar first), renormalised.  Each block is used up before the
// next is drawn (four samples live at a time).  NE > 0 (fp32): the results are staged through the LDS column `col` ([13][NE] floats, the
// lane's own) as they are formed and read back at the end, so that the copy does not sit in registers beside the Philox rounds.
template <typename T, int KW, int NE = 0>
__device__ __forceinline__ void sensor_perturb(uint32_t seed_lo, uint32_t seed_hi, const NoiseSig& S, int64_t gid, int32_t episode, int32_t step, Env<T, KW>& c,
                                               float* col = nullptr) {
  static_assert(NE == 0 || sizeof(T) == 4, "the LDS column holds floats");
  float n[4];
  noise_block(seed_lo, seed_hi, gid, episode, step, 0u, n);
  c.px = fma_(T(S.p), T(n[0]), c.px); c.py = fma_(T(S.p), T(n[1]), c.py); c.pz = fma_(T(S.p), T(n[2]), c.pz);
  c.vx = fma_(T(S.v), T(n[3]), c.vx);
  if constexpr (NE > 0) { col[0] = c.px; col[NE] = c.py; col[2 * NE] = c.pz; col[3 * NE] = c.vx; asm volatile("" ::: "memory"); }
  noise_block(seed_lo, seed_hi, gid, episode, step, 1u, n);
  c.vy = fma_(T(S.v), T(n[0]), c.vy); c.vz = fma_(T(S.v), T(n[1]), c.vz);
  c.wx = fma_(T(S.w), T(n[2]), c.wx); c.wy = fma_(T(S.w), T(n[3]), c.wy);
  if constexpr (NE > 0) { col[4 * NE] = c.vy; col[5 * NE] = c.vz; col[6 * NE] = c.wx; col[7 * NE] = c.wy; asm volatile("" ::: "memory"); }
  noise_block(seed_lo, seed_hi, gid, episode, step, 2u, n);
  c.wz = fma_(T(S.w), T(n[0]), c.wz);
  const T ha = T(0.5f * S.a);
  const T dx = ha * T(n[1]), dy = ha * T(n[2]), dz = ha * T(n[3]);
  const T qw = fma_(-c.qz, dz, fma_(-c.qy, dy, fma_(-c.qx, dx, c.qw)));
  const T qx = fma_(-c.qz, dy, fma_(c.qy, dz, fma_(c.qw, dx, c.qx)));
  const T qy = fma_(-c.qx, dz, fma_(c.qz, dx, fma_(c.qw, dy, c.qy)));
  const T qz = fma_(-c.qy, dx, fma_(c.qx, dy, fma_(c.qw, dz, c.qz)));
  const T rn = rsqrt_(fma_(qw, qw, fma_(qx, qx, fma_(qy, qy, qz * qz))));
  c.qw = qw * rn; c.qx = qx * rn; c.qy = qy * rn; c.qz = qz * rn;
  if constexpr (NE > 0) {
    col[8 * NE] = c.wz; col[9 * NE] = c.qw; col[10 * NE] = c.qx; col[11 * NE] = c.qy; col[12 * NE] = c.qz;
    asm volatile("" ::: "memory");   // the copy is read back from the column: nothing is forwarded in registers
    c.px = col[0]; c.py = col[NE]; c.pz = col[2 * NE]; c.vx = col[3 * NE]; c.vy = col[4 * NE]; c.vz = col[5 * NE]; c.wx = col[6 * NE];
    c.wy = col[7 * NE]; c.wz = col[8 * NE]; c.qw = col[9 * NE]; c.qx = col[10 * NE]; c.qy = col[11 * NE]; c.qz = col[12 * NE];
  }
}
// What the cold, host-launched kernels (reset, observe) take: a wave-uniform switch, the sigmas and the key's seed / first global id.
struct NoiseRt { NoiseSig s; uint32_t seed_lo, seed_hi; int64_t gid0; int32_t on; };

// ---- actuation latency: the draw, and the two accesses of a step -------------------------------------------------------------
constexpr uint32_t kDelayBlock = 0x4C540000u;   // counter word 3 of the d draw ("LT"; resets use 0..4, randomisation 0x4452...., noise 0x4E......)
// env i's slot k sits at delay_slot(i) + 64 k (float4 units); its word at delay_word(D)[i]
__device__ __forceinline__ size_t delay_slot(int i) { return size_t(i >> 6) * (AMENV_MAX_ACTION_DELAY * 64) + size_t(i & 63); }
__device__ __forceinline__ int32_t* delay_word(const DelayArg<true>& D) { return reinterpret_cast<int32_t*>(D.h + size_t(D.n_pad) * AMENV_MAX_ACTION_DELAY); }
// d of (env, episode): one Philox block, integer arithmetic only (w0's top 16 bits times the range's width, <= 9: no overflow)
__device__ __forceinline__ int delay_draw(uint32_t seed_lo, uint32_t seed_hi, const DelayArg<true>& D, int64_t gid, int32_t episode) {
  uint32_t w[4];
  philox4x32_10(seed_lo, seed_hi, uint32_t(uint64_t(gid)), uint32_t(uint64_t(gid) >> 32), uint32_t(episode), kDelayBlock, w);
  return D.lo + int(((w[0] >> 16) * uint32_t(D.span)) >> 16);
}
// Before dynamics(): the env's word, then ONE slot -- the row given d steps ago, which replaces the given row unless d = 0 (the load is
// unconditional: with d = 0 it reads the slot the given row is about to enter; padding lanes own valid slots as of the blob).
__device__ __forceinline__ void delay_apply(const DelayArg<true>& D, int i, DelayLane& dl, float* act) {
  const int32_t m = delay_word(D)[i];
  dl.d = m & 15; dl.head = (m >> 4) & 7;
  const float4 r = D.h[delay_slot(i) + 64 * ((dl.head - dl.d) & 7)];
  if (dl.d != 0) { act[0] = r.x; act[1] = r.y; act[2] = r.z; act[3] = r.w; }
}
// The same with the action history: where two rows are appended, the row given in the step before -- slot (head - 1) & 7 as it is
// BEFORE this step's push -- is loaded next to the delayed row (independent addresses: no further dependent trip).  hr.g0 is the caller's.
__device__ __forceinline__ void delay_apply(const DelayArg<true>& D, int i, DelayLane& dl, float* act, HistRows& hr) {
  const int32_t m = delay_word(D)[i];
  dl.d = m & 15; dl.head = (m >> 4) & 7;
  const float4* p = D.h + delay_slot(i);
  const float4 r = p[64 * ((dl.head - dl.d) & 7)];
  hr.n = D.hist;
  hr.g1 = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
  if (D.hist > 1) hr.g1 = p[64 * ((dl.head - 1) & 7)];
  if (dl.d != 0) { act[0] = r.x; act[1] = r.y; act[2] = r.z; act[3] = r.w; }
}
// columns OD .. OD + 4 n of a row (dst points at column OD; float4 stores where the row is 16-byte aligned)
template <bool VEC>
__device__ __forceinline__ void hist_put(float* dst, const HistRows& hr) {
  if constexpr (VEC) {
    if (hr.n > 0) reinterpret_cast<float4*>(dst)[0] = hr.g0;
    if (hr.n > 1) reinterpret_cast<float4*>(dst)[1] = hr.g1;
  } else {
    if (hr.n > 0) { dst[0] = hr.g0.x; dst[1] = hr.g0.y; dst[2] = hr.g0.z; dst[3] = hr.g0.w; }
    if (hr.n > 1) { dst[4] = hr.g1.x; dst[5] = hr.g1.y; dst[6] = hr.g1.z; dst[7] = hr.g1.w; }
  }
}
// After the step: the given row enters the history (ONE slot), or, where a new episode starts (the caller has put its d into dl), all 8
// slots become the hover row; then the word.
__device__ __forceinline__ void delay_push(const DelayArg<true>& D, int i, DelayLane& dl, const float4 given, bool was_reset) {
  float4* p = D.h + delay_slot(i);
  if (was_reset) {
#pragma unroll
    for (int k = 0; k < AMENV_MAX_ACTION_DELAY; k++) p[64 * k] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    dl.head = 0;
  } else {
    p[64 * dl.head] = given;
    dl.head = (dl.head + 1) & 7;
  }
  delay_word(D)[i] = dl.d | (dl.head << 4);
}

// WaypointQuadEnv.reset (rl_env_scaledObs.py:40-79) with the DESIGN.md draw table.  All draws
// are formed in fp32 with explicit fmaf so the CPU oracle reproduces them bit for bit.
// The 12 Philox words of one reset, computed by the resetting lane itself (three blocks in sequence).
__device__ __forceinline__ void reset_words_serial(const ColdParams& P, int64_t gid, int32_t episode, uint32_t* r) {
#pragma unroll
  for (uint32_t b = 0; b < 3; b++)
    philox4x32_10(P.seed_lo, P.seed_hi, uint32_t(uint64_t(gid)), uint32_t(uint64_t(gid) >> 32), uint32_t(episode), b, &r[4 * b]);
}

// Same 12 words, wave-cooperative: episode ends are rare, so when a wave enters the reset path usually ONE lane
// needs words while 63 idle.  For each resetting lane (scalar loop) lanes 0..2 each run one of the three Philox
// blocks (block index = lane id) and the 12 results are handed to the owner through v_readlane: one block of
// latency instead of three (the 32x32->64 multiplies are quarter rate).  Must be called by ALL lanes of the wave.
__device__ __forceinline__ void reset_words_wave(const ColdParams& P, bool need, int64_t gid, int32_t episode, uint32_t* r) {
  unsigned long long m = __ballot(need);
  const int lane = int(threadIdx.x & 63);
  const uint32_t g_lo = uint32_t(uint64_t(gid)), g_hi = uint32_t(uint64_t(gid) >> 32);
  while (m) {  // wave-uniform
    const int l = __builtin_ctzll(m);
    m &= m - 1;
    const uint32_t c0 = __builtin_amdgcn_readlane(g_lo, l), c1 = __builtin_amdgcn_readlane(g_hi, l);
    const uint32_t c2 = uint32_t(__builtin_amdgcn_readlane(episode, l));
    uint32_t w[4];
    philox4x32_10(P.seed_lo, P.seed_hi, c0, c1, c2, uint32_t(lane), w);   // lanes 0,1,2 hold blocks 0,1,2
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t v = __builtin_amdgcn_readlane(w[k], b);
        if (lane == l) r[4 * b + k] = v;
      }
  }
}

// WaypointQuadEnv.reset (rl_env_scaledObs.py:40-79) from its 12 Philox words r[] (DESIGN.md draw table).  All draws
// are formed in fp32 with explicit fmaf so the CPU oracle reproduces them bit for bit.
template <typename T, int KW>
__device__ __forceinline__ void reset_from_words(const ColdParams& P, int K, Env<T, KW>& e, const uint32_t* r) {
  const float PIF = 3.14159274101257324f;
  const float sx = fmaf(2.0f, u01(r[0]), -1.0f);                        // :44
  const float sy = fmaf(2.0f, u01(r[1]), -1.0f);
  const float sz = fmaf(1.0f, u01(r[3]), 1.0f);                         // :45
  const float sel0 = u01(r[4]), sel1 = u01(r[5]);                       // :63,65
  const float ex = fmaf(2.0f, u01(r[6]), -1.0f);                        // utils2/utils.py:15-16
  const float ey = fmaf(2.0f, u01(r[7]), -1.0f);
  const float ez = fmaf(2.5f, u01(r[9]), 0.5f);
  const uint32_t axis = r[10] % 3u;                                     // utils2/utils.py:32
  const float fyaw = fmaf(2.0f * PIF, u01(r[11]), -PIF);                // :72
  const int kind = sel0 < 0.3f ? 0 : (sel1 < 0.6f ? 1 : 2);
#pragma unroll
  for (int k = 1; k <= KW; k++) {
    if (k > K) break;
    float wx, wy, wz;
    if (kind == 2) {                                                    // helical, utils2/utils.py:61-95
      wx = fmaf(0.8f, P.traj_cos[k - 1], sx);
      wy = fmaf(0.8f, P.traj_sin[k - 1], sy);
      wz = fmaxf(fmaf(float(k), 0.4f, sz), 0.2f);
    } else {                                                            // linear / curved, :12-57
      const float t = float(k) / float(K);
      wx = fmaf(t, ex - sx, sx); wy = fmaf(t, ey - sy, sy); wz = fmaf(t, ez - sz, sz);
      if (kind == 1) {
        const float s = P.traj_sin[k - 1];
        if (axis == 0) wz = wz + s; else if (axis == 1) wy = wy + s; else wx = wx + s;
        wz = fmaxf(wz, 0.2f);
      }
    }
    e.wp[k - 1][0] = T(wx); e.wp[k - 1][1] = T(wy); e.wp[k - 1][2] = T(wz);
  }
  e.px = T(sx); e.py = T(sy); e.pz = T(sz);
  e.vx = e.vy = e.vz = T(0);
  e.qw = T(1); e.qx = e.qy = e.qz = T(0);                               // quadcopter.py:28-38, attitude (0,0,0)
  e.wx = e.wy = e.wz = T(0);
  e.final_yaw = T(fyaw);
#pragma unroll
  for (int k = 0; k < AMENV_MAX_JOINTS; k++) { e.th[k] = T(0); e.thd[k] = T(0); }     // arm at home (the caller sets the tool offset)
  e.last_distance = T(-1);                                              // :76 None
  e.ep_return = T(0);
  e.step = 0; e.counter = 0; e.flags = 0;                               // :55-59,74-77
  e.episode += 1;
}

template <typename T, int KW>
__device__ __forceinline__ void reset_env(const ColdParams& P, int K, bool v1, Env<T, KW>& e, int64_t gid) {
  uint32_t r[12];
  reset_words_serial(P, gid, e.episode, r);
  if (v1) reset_from_words_v1<T, KW>(K, e, r);
  else reset_from_words<T, KW>(P, K, e, r);
}

}  // namespace amenv_dev
