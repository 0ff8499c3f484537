// amenv_eval_policy.hpp -- closed-loop policy EVALUATION in one launch (amenv_evaluate_policy): the evaluation forms of the two
// one-lane-per-env rollout kernels, rollout_policy_kernel_rigid (amenv_rigid_policy.hpp) and rollout_policy_kernel_lane (amenv_lane_policy.hpp).
//   * the same closed loop: the MLP half (policy_mlp_waves, amenv_policy_mlp.hpp: the rollout kernels' call with the exit test on), five barriers
//     per step, the Philox keying (seed, global env id, draw0 + t) and step_lane -- applied action for applied action the trajectories are the
//     rollout kernels', bit for bit;
//   * the action: `deterministic` != 0 applies clip(mean) (no draw), otherwise the rollout's sample clip(mean + std z);
//   * nothing per step goes to global memory (the action delay's ring, which is env state, aside): no obs / actions / logp / values / rewards /
//     dones / terminal rows.  The MLP input tile in LDS is written every step.  The critic half runs (it is the rollout's code), its value is not read;
//   * per-env accounting in registers: a lane counts the first `quota` episodes that END in its env (the one running at entry included): the fp32
//     episode return as step_lane hands it out goes into two fp64 sums (sum, sum of squares), the length into an int32 sum, and the counters
//     episodes / success / crashed / out_of_bounds / truncated go up by one where the end bits carry the AMENV_INFO_* bit (not exclusive).
//     After its quota a lane keeps stepping (the barriers need it) and adds nothing;
//   * early exit per workgroup (THE EXIT PROTOCOL, amenv_policy_mlp.hpp, holds the argument); steps_run = max over workgroups of the steps executed;
//   * one workgroup shape: 16 envs for the rigid vehicles (the finest early exit), 64 envs (one env wavefront) for the arm;
//   * the Monitor totals (amenv_stats) are not touched: no accumulate_stats call.
// The env state goes back to the blob at the end as the rollout kernels store it: the handle is wherever its lanes stopped.
#pragma once
#include "amenv_lane_policy.hpp"
#include "amenv_rigid_policy.hpp"

namespace amenv_dev {

struct EvalArg {
  int32_t deterministic;   // != 0: the applied action is clip(mean)
  int32_t quota;           // episodes counted per env
  double* returns;         // [N][2]: sum, sum of squares of the counted episodes' returns
  int32_t* counts;         // [N][AMENV_EVAL_COUNT_COLS]: episodes, length_sum, success, crashed, out_of_bounds, truncated
  int32_t* steps_run;      // [1]: atomicMax of every workgroup's executed steps (zeroed on the stream in front of the launch)
};

// one lane's accumulators
struct EvalAcc {
  double ret = 0.0, ret2 = 0.0;
  int32_t episodes = 0, length = 0, success = 0, crashed = 0, oob = 0, truncated = 0;
  __device__ __forceinline__ void add(uint32_t bits, int ep_len, float ep_ret) {
    const double r = double(ep_ret);
    ret += r; ret2 += r * r;
    episodes += 1; length += ep_len;
    success += (bits & AMENV_INFO_SUCCESS) ? 1 : 0;
    crashed += (bits & AMENV_INFO_CRASHED) ? 1 : 0;
    oob += (bits & AMENV_INFO_OOB) ? 1 : 0;
    truncated += (bits & AMENV_INFO_TRUNCATED) ? 1 : 0;
  }
  __device__ __forceinline__ void store(const EvalArg& E, int i) const {
    E.returns[size_t(i) * 2] = ret; E.returns[size_t(i) * 2 + 1] = ret2;
    int32_t* c = E.counts + size_t(i) * AMENV_EVAL_COUNT_COLS;
    c[0] = episodes; c[1] = length; c[2] = success; c[3] = crashed; c[4] = oob; c[5] = truncated;
  }
};

// The arm kernel's env code fills the register file (amenv_lane_policy.hpp: 254..256 VGPRs), so its lanes keep their sums in LDS, each lane its own
// column (no barrier: nobody else reads them), touched at episode ends only; the episode count, compared every step, stays in a register
template <int NE>
struct EvalAccLds {
  double* d;      // this lane's column of [2][NE] doubles: sum, sum of squares
  int32_t* c;     // this lane's column of [5][NE] ints: length, success, crashed, out_of_bounds, truncated
  int32_t episodes = 0;
  __device__ __forceinline__ EvalAccLds(double* d_, int32_t* c_) : d(d_), c(c_) {
    d[0] = 0.0; d[NE] = 0.0;
#pragma unroll
    for (int k = 0; k < 5; k++) c[k * NE] = 0;
  }
  __device__ __forceinline__ void add(uint32_t bits, int ep_len, float ep_ret) {
    const double r = double(ep_ret);
    d[0] += r; d[NE] += r * r;
    episodes += 1; c[0] += ep_len;
    c[NE] += (bits & AMENV_INFO_SUCCESS) ? 1 : 0;
    c[2 * NE] += (bits & AMENV_INFO_CRASHED) ? 1 : 0;
    c[3 * NE] += (bits & AMENV_INFO_OOB) ? 1 : 0;
    c[4 * NE] += (bits & AMENV_INFO_TRUNCATED) ? 1 : 0;
  }
  __device__ __forceinline__ void store(const EvalArg& E, int i) const {
    E.returns[size_t(i) * 2] = d[0]; E.returns[size_t(i) * 2 + 1] = d[NE];
    int32_t* o = E.counts + size_t(i) * AMENV_EVAL_COUNT_COLS;
    o[0] = episodes;
#pragma unroll
    for (int k = 0; k < 5; k++) o[1 + k] = c[k * NE];
  }
};

// Rigid vehicles (4 or 6 rotors, fp32, every task, every admitted switch set, with or without the frozen normaliser): NE = 16
template <int NROT, int KW, int VAR, bool NORM, unsigned DYN = 0>
__global__ __launch_bounds__(320) void evaluate_policy_kernel_rigid(void* __restrict__ blob, uint32_t tile_bytes, int32_t n_envs, int max_steps, const PolicyIO io,
                                                                    const HotParams<float, NROT> P, const ColdParams C, const NormArg N, const DynArg<float, NROT, DYN> DA,
                                                                    const EvalArg E) {
  static_assert(dyn_admitted<float, 0>(DYN), "a switch set that is not built (amenv_model.hpp)");
  constexpr bool DR = (DYN & kDynDr) != 0, LAG = (DYN & kDynLag) != 0, NOISE = (DYN & kDynNoise) != 0, DELAY = (DYN & kDynDelay) != 0;
  constexpr int OD = ObsDim<VAR, 0>::value, AD = 4, NE = 16;
  __shared__ __attribute__((aligned(16))) __bf16 xin[NE * kXS];
  __shared__ __attribute__((aligned(16))) __bf16 xlo[NE * kXS];
  __shared__ __attribute__((aligned(16))) __bf16 h1[2 * NE * kH1S];
  __shared__ __attribute__((aligned(16))) __bf16 h2[2 * NE * kH2S];
  __shared__ __attribute__((aligned(16))) float meanb[NE * 4];
  __shared__ float valb[NE];
  __shared__ double md[NORM ? 2 * OD : 1];                                // entry statistics: mean | 1 / sqrt(var + eps)
  __shared__ float wl[LAG ? (2 * NROT + 2) * NE : 1];                     // rotor states | dynamics factors (amenv_rigid_policy.hpp)
  constexpr bool kNoiseLds = NOISE && NORM;
  constexpr bool kFailLds = DR && NORM;                                   // rotor failure: the NORM forms keep the lanes' plans in LDS
  __shared__ int32_t fkl[kFailLds ? 2 * NE : 1];                          // [2][NE] words: key, f; each lane reads and writes its own column
  __shared__ float zl[kNoiseLds ? 13 * NE : 1];
  __shared__ int pend;                                                    // the exit protocol's word (policy_mlp_waves)
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  const int lane = int(threadIdx.x) & 63;
  if constexpr (NORM) {
    for (int j = int(threadIdx.x); j < OD; j += int(blockDim.x)) { md[j] = N.buf[j]; md[OD + j] = 1.0 / sqrt(N.buf[OD + j] + N.eps); }
    __syncthreads();
  }
  if (wave < 4) { policy_mlp_waves<NE, true, 4, true>(io, wave, lane, max_steps, xin, xlo, h1, h2, meanb, valb, &pend); return; }
  // ---- the env wavefront: lanes 0..15 an env each; the others only pass the barriers
  const int el = lane;
  const bool mine = el < NE;
  const int i = int(blockIdx.x) * NE + (mine ? el : 0);
  const int tl = i & 63;
  const bool active = mine && i < n_envs;
  char* tile = static_cast<char*>(blob) + size_t(i >> 6) * tile_bytes;
  const int K = KW == 1 ? 1 : P.K;
  Env<float, KW> e;
  DynFac<float, NROT, DR> df;
  FailLane fl{-1, 0.0f};                                          // rotor failure: the episode's plan, spent when the factor holds it
  float std_a[AD];
  float o[kObsDimMax];
  constexpr bool kHist = DELAY && !NORM;
  std::conditional_t<kHist, HistRows, NoHist> hr;
  int W = OD;
  if constexpr (kHist) { hr.n = DA.D.hist; hr.hover(); W = OD + 4 * hr.n; }
  auto publish_obs = [&]() {                                      // observation row -> (two bf16 parts) the MLP input tile
    __bf16* xr = xin + el * kXS;
    __bf16* xl = xlo + el * kXS;
#pragma unroll
    for (int j = 0; j < OD; j++) {
      float v = o[j];
      if constexpr (NORM) {   // obsnorm_apply_kernel's arithmetic
        const float x = float((double(o[j]) - md[j]) * md[OD + j]);
        v = x < -N.clip ? -N.clip : (x > N.clip ? N.clip : x);
      }
      const __bf16 hi = (__bf16)v; xr[j] = hi; xl[j] = (__bf16)(v - float(hi));
    }
    if constexpr (kHist) {
      const float g[8] = {hr.g0.x, hr.g0.y, hr.g0.z, hr.g0.w, hr.g1.x, hr.g1.y, hr.g1.z, hr.g1.w};
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (j < 4 * hr.n) { const __bf16 hi = (__bf16)g[j]; xr[OD + j] = hi; xl[OD + j] = (__bf16)(g[j] - float(hi)); }
    }
  };
  if (mine) {
    load_env<float, KW, 0>(K, tile, tl, e);
    if constexpr (DR && !LAG) df = dr_factors<float, NROT>(P, C, DA.R.r, C.gid0 + i, e.episode);
    if constexpr (LAG) {
#pragma unroll
      for (int r = 0; r < NROT; r++) wl[r * NE + el] = DA.L.w[lag_slot<NROT>(i) + r * 64];
      LagLds<NROT, NE, true>{wl + el, 0.0f, 0.0f}.put(dr_factors<float, NROT>(P, C, DA.R.r, C.gid0 + i, e.episode));
    }
    if constexpr (DR) {
      if (DA.R.x.ctl != 0u) fl = fail_draw<NROT>(C, DA.R.x, C.gid0 + i, e.episode);
      if constexpr (kFailLds) fail_put<NE>(fkl + el, fl);
    }
    const uint4* ac = io.pack + size_t(4) * (kPolFrags + kPolBias) * 64;   // policy_pack_kernel's per-entry {std, log_std}
#pragma unroll
    for (int c = 0; c < AD; c++) std_a[c] = __uint_as_float(ac[c].x);
    if constexpr (NOISE) {
      Env<float, KW> c = e;
      sensor_perturb<float, KW, kNoiseLds ? NE : 0>(C.seed_lo, C.seed_hi, DA.Z.s, C.gid0 + i, e.episode, e.step, c, zl + el);
      if constexpr (VAR == VAR_V1) observe_v1<float, KW>(P.raw_obs != 0, c, o); else observe<float, KW>(K, c, o);
    } else {
      if constexpr (VAR == VAR_V1) observe_v1<float, KW>(P.raw_obs != 0, e, o); else observe<float, KW>(K, e, o);
    }
    __bf16* xr = xin + el * kXS;
    __bf16* xl = xlo + el * kXS;
#pragma unroll
    for (int j = OD; j < 32; j++) { xr[j] = (__bf16)(j == W ? 1.0f : 0.0f); xl[j] = (__bf16)0.0f; }   // bias column (behind the history's), K padding
    if constexpr (kHist) {
      const int head = (delay_word(DA.D)[i] >> 4) & 7;
      const float4* p = DA.D.h + delay_slot(i);
      if (hr.n > 0) hr.g0 = p[64 * ((head - 1) & 7)];
      if (hr.n > 1) hr.g1 = p[64 * ((head - 2) & 7)];
    }
    publish_obs();
  }
  const int64_t gid = C.gid0 + i;
  const uint32_t g_lo = uint32_t(uint64_t(gid)), g_hi = uint32_t(uint64_t(gid) >> 32);
  bool any_reset = false;
  const StepIO sio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const ArmArg<float, 0> AA{0};
  EvalAcc acc;
  if (lane == 0) pend = __ballot(active) != 0ull ? 1 : 0;         // (w0): quota > 0, so every active env is pending
  int t = 0;
  for (; t < max_steps; t++) {
    __syncthreads();   // (B0) observation tile published
    if (!eval_pending(&pend)) break;                              // the exit protocol (policy_mlp_waves): the MLP wavefronts leave in this iteration too
    __syncthreads();   // (B1)
    __syncthreads();   // (B2)
    __syncthreads();   // (B3)
    __syncthreads();   // (B4) action means of this lane's env are in LDS
    bool short_of_quota = false;
    if (mine) {
      const float4 m = *reinterpret_cast<const float4*>(meanb + el * 4);
      float act[AD] = {m.x, m.y, m.z, m.w};
      if (E.deterministic == 0) {   // the rollout's sample: raw = mean + std z
        float z[4];
        policy_normal4(io, g_lo, g_hi, io.draw0 + uint32_t(t), 0u, z);
#pragma unroll
        for (int c = 0; c < AD; c++) act[c] = fma_(std_a[c], z[c], act[c]);
      }
#pragma unroll
      for (int c = 0; c < AD; c++) act[c] = policy_clip(act[c], c);
      DelayLane dl; float4 given;
      if constexpr (DELAY) {
        given = make_float4(act[0], act[1], act[2], act[3]);
        if constexpr (kHist) { hr.g0 = given; delay_apply(DA.D, i, dl, act, hr); } else delay_apply(DA.D, i, dl, act);
      }
      if constexpr (DR) rate_apply(P, DA.R.q, e, act);   // body-rate actions: behind the clipped action and the latency, in front of the step
      if constexpr (kFailLds) fail_hit_lds<NROT, NE>(fkl + el, e.step, LAG ? nullptr : df.s, wl + el);   // rotor failure: the step field as this step finds it
      else if constexpr (DR && LAG) fail_hit_scol<NROT, NE>(fl, e.step, wl + el);
      else if constexpr (DR) fail_hit<float, NROT>(fl, e.step, df.s);
      float reward; bool was_reset; int ep_len; float ep_ret;
      LagLds<NROT, NE, LAG> lg;
      if constexpr (LAG) { lg.col = wl + el; lg.a_up = DA.L.a_up; lg.a_down = DA.L.a_down; }
      uint32_t bits;
      if constexpr (kNoiseLds)
        bits = step_lane<float, NROT, KW, VAR, 0, 0, NoXchg, DR, LagLds<NROT, NE, LAG>, NoiseLds<NE>>(P, C, AA, e, act, i, active, reward, o, sio, tile, tl, any_reset, was_reset, ep_len,
                                                                                                     ep_ret, NoXchg{}, df, &lg, NoiseLds<NE>{DA.Z.s, zl + el});
      else
        bits = step_lane<float, NROT, KW, VAR, 0, 0, NoXchg, DR, LagLds<NROT, NE, LAG>, NoiseArg<NOISE>>(P, C, AA, e, act, i, active, reward, o, sio, tile, tl, any_reset, was_reset, ep_len,
                                                                                                        ep_ret, NoXchg{}, df, &lg, noise_of(DA), &hr);
      if constexpr (DR && !LAG) { if (was_reset) df = dr_factors<float, NROT>(P, C, DA.R.r, gid, e.episode); }
      if constexpr (LAG) {
        if (was_reset) {
#pragma unroll
          for (int r = 0; r < NROT; r++) wl[r * NE + el] = DA.L.w[size_t(NROT) * DA.L.n_pad + r];
          lg.put(dr_factors<float, NROT>(P, C, DA.R.r, gid, e.episode));
        }
      }
      if constexpr (DR) {
        if (was_reset && DA.R.x.ctl != 0u) {   // the new episode's plan
          const FailLane nf = fail_draw<NROT>(C, DA.R.x, gid, e.episode);
          if constexpr (kFailLds) fail_put<NE>(fkl + el, nf); else fl = nf;
        }
      }
      if constexpr (DELAY) {
        if (was_reset) { dl.d = delay_draw(C.seed_lo, C.seed_hi, DA.D, gid, e.episode); if constexpr (kHist) hr.hover(); }
        delay_push(DA.D, i, dl, given, was_reset);
      }
      any_reset |= was_reset;
      const bool is_done = active && (bits & (AMENV_INFO_TERMINATED | AMENV_INFO_TRUNCATED)) != 0;
      if (is_done && acc.episodes < E.quota) acc.add(bits, ep_len, ep_ret);
      short_of_quota = active && acc.episodes < E.quota;
      publish_obs();                                              // the next step's MLP input
    }
    const bool wg_pending = __ballot(short_of_quota) != 0ull;
    if (lane == 0) pend = wg_pending ? 1 : 0;                     // (w): read by everyone behind B0 of step t + 1
  }
  if (lane == 0) atomicMax(E.steps_run, t);
  if (mine) {
    if (active) acc.store(E, i);
    store_env_step<float, KW, 0>(tile, tl, e, K);
    if (any_reset) store_env_episode<float, KW>(K, tile, tl, e);
    if constexpr (LAG) {
#pragma unroll
      for (int r = 0; r < NROT; r++) DA.L.w[lag_slot<NROT>(i) + r * 64] = wl[r * NE + el];
    }
  }
}

// The 6-rotor vehicle with an arm (1..3 public joints, 1..4 waypoints): 64 envs per workgroup, one env wavefront
template <int KW, int PNJ>
__global__ __launch_bounds__(320) void evaluate_policy_kernel_lane(void* __restrict__ blob, uint32_t tile_bytes, int32_t n_envs, int max_steps, const PolicyIO io,
                                                                   const HotParams<float, 6> P, const ColdParams C, const ArmArg<float, 3> AA, const EvalArg E) {
  constexpr int NROT = 6, OD = 29, AD = 7, NE = 64, NJ = 3;
  static_assert(PNJ >= 1 && PNJ <= 3, "1..3 public joints");
  __shared__ __attribute__((aligned(16))) __bf16 xin[NE * kXS];
  __shared__ __attribute__((aligned(16))) __bf16 h1[2 * NE * kH1S];
  __shared__ __attribute__((aligned(16))) __bf16 h2[2 * NE * kH2S];
  __shared__ __attribute__((aligned(16))) float meanb[NE * 8];
  __shared__ float valb[NE];
  __shared__ double accd[2 * NE];                                         // the lanes' sums (EvalAccLds)
  __shared__ int32_t accc[5 * NE];
  __shared__ int pend;                                                    // the exit protocol's word (policy_mlp_waves)
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  const int lane = int(threadIdx.x) & 63;
  if (wave < 4) { policy_mlp_waves<NE, false, 8, true>(io, wave, lane, max_steps, xin, nullptr, h1, h2, meanb, valb, &pend); return; }
  // ---- the env wavefront: one lane per env
  const int el = lane;
  const int i = int(blockIdx.x) * NE + el;
  const bool active = i < n_envs;
  char* tile = static_cast<char*>(blob) + size_t(i >> 6) * tile_bytes;
  const int K = KW == 1 ? 1 : P.K;
  Env<float, KW> e;
  load_env<float, KW, NJ>(K, tile, lane, e);
  float std_a[AD];
  {
    const uint4* ac = io.pack + size_t(4) * (kPolFrags + kPolBias) * 64;   // policy_pack_kernel's last block (amenv_lane_policy.hpp)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint4 v = ac[c];
      std_a[c] = __uint_as_float(v.x);
      if (c < 3) std_a[4 + c] = __uint_as_float(v.z);
    }
  }
  const int64_t gid = C.gid0 + i;
  const uint32_t g_lo = uint32_t(uint64_t(gid)), g_hi = uint32_t(uint64_t(gid) >> 32);
  const bool ee_task = P.ee_task != 0;
  float o[kObsDimMax];
  update_tool_offset<float, KW, false>(AA.p, e);
  observe<float, KW, true>(K, e, o, ee_task);
  observe_joints<float, KW>(e, o);
  auto publish_obs = [&]() {                                     // observation row -> (bf16) the MLP's input tile
    __bf16* xr = xin + el * kXS;
#pragma unroll
    for (int j = 0; j < OD; j++) xr[j] = (__bf16)o[j];
  };
  { __bf16* xr = xin + el * kXS; xr[OD] = (__bf16)1.0f; xr[OD + 1] = (__bf16)0.0f; xr[OD + 2] = (__bf16)0.0f; }   // bias column, K padding
  publish_obs();
  bool any_reset = false;
  const StepIO sio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  EvalAccLds<NE> acc(accd + el, accc + el);
  if (lane == 0) pend = __ballot(active) != 0ull ? 1 : 0;         // (w0): quota > 0, so every active env is pending
  int t = 0;
  for (; t < max_steps; t++) {
    __syncthreads();   // (B0) observation tile published
    if (!eval_pending(&pend)) break;                              // the exit protocol (policy_mlp_waves): the MLP wavefronts leave in this iteration too
    __syncthreads();   // (B1)
    __syncthreads();   // (B2)
    __syncthreads();   // (B3)
    __syncthreads();   // (B4) action means of this lane's env are in LDS
    float act[AD];
    {
      const float4 m0 = *reinterpret_cast<const float4*>(meanb + el * 8), m1 = *reinterpret_cast<const float4*>(meanb + el * 8 + 4);
      act[0] = m0.x; act[1] = m0.y; act[2] = m0.z; act[3] = m0.w; act[4] = m1.x; act[5] = m1.y; act[6] = m1.z;
    }
    if (E.deterministic == 0) {   // the rollout's sample: Philox block 0 -> wrench entries, block 1 -> joints
      float z[8];
      policy_normal4(io, g_lo, g_hi, io.draw0 + uint32_t(t), 0u, z);
      policy_normal4(io, g_lo, g_hi, io.draw0 + uint32_t(t), 1u, z + 4);
#pragma unroll
      for (int c = 0; c < 4 + PNJ; c++) act[c] = fma_(std_a[c], z[c], act[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) act[c] = policy_clip(act[c], c);
#pragma unroll
    for (int c = 0; c < 3; c++) act[4 + c] = c < PNJ ? clamp_(act[4 + c], -1.0f, 1.0f) : 0.0f;   // a phantom joint: no command
    float reward; bool was_reset; int ep_len; float ep_ret;
    uint32_t bits;
    if constexpr (KW == 1) {
      bits = step_lane<float, NROT, KW, VAR_V2, NJ>(P, C, AA, e, act, i, active, reward, o, sio, tile, lane, any_reset, was_reset, ep_len, ep_ret);
    } else {   // K made opaque per step (amenv_lane_policy.hpp)
      HotParams<float, NROT> Pk = P;
      int k = Pk.K;
      asm volatile("" : "+s"(k));
      Pk.K = k;
      bits = step_lane<float, NROT, KW, VAR_V2, NJ>(Pk, C, AA, e, act, i, active, reward, o, sio, tile, lane, any_reset, was_reset, ep_len, ep_ret);
    }
    any_reset |= was_reset;
    const bool is_done = active && (bits & (AMENV_INFO_TERMINATED | AMENV_INFO_TRUNCATED)) != 0;
    if (is_done && acc.episodes < E.quota) acc.add(bits, ep_len, ep_ret);
    publish_obs();                                                // the next step's MLP input
    const bool wg_pending = __ballot(active && acc.episodes < E.quota) != 0ull;
    if (lane == 0) pend = wg_pending ? 1 : 0;                     // (w): read by everyone behind B0 of step t + 1
  }
  if (lane == 0) atomicMax(E.steps_run, t);
  if (active) acc.store(E, i);
  if constexpr (KW > 1) asm volatile("" : "+v"(tile));
  store_env_step<float, KW, NJ>(tile, lane, e, K);
  if (any_reset) store_env_episode<float, KW>(K, tile, lane, e);
}

}  // namespace amenv_dev
