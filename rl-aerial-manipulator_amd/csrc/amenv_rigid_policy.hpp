// amenv_rigid_policy.hpp -- closed-loop rollout in ONE launch for the rigid vehicles (4 or 6 rotors, fp32) on every task the step kernels
// serve: the v1 tasks (17-D observation, 1..2 waypoints per episode; v1/rl_train_vecN.py trains them) and the v2 task with 1..4 waypoints;
// optionally with the observation normaliser inside the launch (VecNormalize(norm_obs=True, norm_reward=False), v1/rl_train_vecN.py:10-11).
//   * env part: ONE LANE PER ENV, step_lane<float, NROT, KW, VAR, 0> -- the arithmetic of amenv_step's LANE / HELPER kernels, so replaying the
//     recorded clipped actions through amenv_step on such a handle reproduces every row bit for bit.  Tile addressing is by the env index
//     (i & 63), the blob layout is the step kernels';
//   * MLP part: amenv_policy_mlp.hpp's policy_mlp_waves with the two-part first layer (xin / xlo; DESIGN 4g: one bf16 rounding of the input
//     moved a trained controller's action by up to 0.107; normalised inputs reach +-10);
//   * sampling: policy_normal4, block 0 = the four wrench entries; the log-probability is summed in the lane-quad form's association: for the same
//     observation both forms draw the same noise;
//   * workgroup = NE envs: NE = 16 (one 16-env column tile, 256 workgroups at 4096 envs: every CU busy) or NE = 64 EW (EW = 1, 2 env
//     wavefronts; the large-batch shape of amenv_lane_policy.hpp).  Wavefronts 0..3 run the MLPs, wavefronts 4.. the envs; with NE = 16
//     lanes 16..63 of the env wavefront only take part in the barriers.  The C ABI picks NE by batch size.
// NORM: the normaliser's statistics are read ONCE at entry (mean and 1/sqrt(var + eps) in fp64, obsnorm_apply_kernel's arithmetic: the
// published rows are bit-identical to amenv_obsnorm_apply under the entry statistics) and are FROZEN for the launch: buffer rows 0..T, the
// MLP input and the terminal rows are normalised with them.  With `update`, the raw rows 1..T of every active env (post-step, post-reset;
// not row 0, which the previous launch or the initial reset counted; not the terminal rows, as the step-by-step path) are summed per lane in
// fp64, reduced once per env wavefront at the end and added into the buffer's batch-sum slots; obsnorm_merge_kernel follows the launch.
#pragma once
#include "amenv_kernels.hpp"
#include "amenv_obsnorm.hpp"
#include "amenv_policy_mlp.hpp"

namespace amenv_dev {

struct NormArg {
  double* buf;    // amenv_obsnorm buffer (obsnorm_words(OD) doubles) or null (NORM = false)
  float clip;
  double eps;
  int32_t update;  // != 0: add the raw rows 1..T into the batch-sum slots
};

// DR: per-episode dynamics randomisation: factors drawn at entry and again for a lane after its auto-reset.
// LAG: first-order rotor lag.  The NORM forms have no VGPR to spare, so the rotor states of this kernel live in LDS, and with
// them the randomisation's factors ((2 NROT + 2) x NE floats, every lane its own column: no barrier): dynamics() filters them there one
// rotor at a time (LagLds), and the states go back to the handle's side buffer once at the end.
// NOISE: sensor noise: row 0 and every later row are formed from a perturbed copy of the state; the noise comes first and the
// normaliser second (the frozen statistics normalise the noisy row, the `update` sums count the noisy raw rows).  In the NORM forms the
// perturbed copy is staged through LDS (13 x NE floats, every lane its own column: NoiseLds).
// DELAY: per-episode actuation latency: the clipped sample is the GIVEN row; the row given d steps ago is applied.  Nothing of the
// history is held in registers over a step: the env's word and one slot are loaded from the handle's (L2-resident) side buffer in front of
// the dynamics, one slot and the word are stored behind them.  `actions` and `logp` record the policy's own samples.
// The rotor failure and the NORM forms: they sit at the vector-register limit and cannot carry a line more without scratch.  For
// them the failure has instantiations of its own, named by kDynFailForm on top of the switch set (DYN = 17u..31u: a form of THIS kernel, not a
// switch bit -- the argument is the set's DynArg), which a handle runs only while the failure is set; the forms every other handle runs
// (DYN <= 15u) hold none of its code and draw the randomisation as before it.  Without the normaliser there is one form, which carries it.
template <int NROT, int KW, int VAR, bool NORM, int NE, unsigned DYNF = 0>
__global__ __launch_bounds__(256 + (NE < 64 ? 64 : NE)) void rollout_policy_kernel_rigid(void* __restrict__ blob, uint32_t tile_bytes, int32_t n_envs, int n_steps,
                                                                                         const PolicyIO io, unsigned long long* __restrict__ stats,
                                                                                         const HotParams<float, NROT> P, const ColdParams C, const NormArg N,
                                                                                         const DynArg<float, NROT, (DYNF & kDynAll)> DA) {
  constexpr unsigned DYN = DYNF & kDynAll;
  constexpr bool FAIL = !NORM || (DYNF & kDynFailForm) != 0;
  static_assert(DYNF <= kDynAll || (NORM && (DYN & kDynDr) != 0), "the failure's forms: NORM, with the randomisation's block");
  static_assert(dyn_admitted<float, 0>(DYN), "a switch set that is not built (amenv_model.hpp)");
  constexpr bool DR = (DYN & kDynDr) != 0, LAG = (DYN & kDynLag) != 0, NOISE = (DYN & kDynNoise) != 0, DELAY = (DYN & kDynDelay) != 0;
  constexpr bool kFail = DR && FAIL, kOwnKey = FAIL;                       // (without the failure's code the randomisation's draw is as it was, too)
  constexpr int OD = ObsDim<VAR, 0>::value, AD = 4, EW = NE < 64 ? 1 : NE / 64;   // env wavefronts per workgroup
  static_assert(NE == 16 || NE == 64 || NE == 128, "workgroup shapes");
  __shared__ __attribute__((aligned(16))) __bf16 xin[NE * kXS];
  __shared__ __attribute__((aligned(16))) __bf16 xlo[NE * kXS];          // the observation's second bf16 part (x - bf16(x))
  __shared__ __attribute__((aligned(16))) __bf16 h1[2 * NE * kH1S];       // layer-1 activations; layer 3's reuse the front of it
  __shared__ __attribute__((aligned(16))) __bf16 h2[2 * NE * kH2S];
  __shared__ __attribute__((aligned(16))) float meanb[NE * 4];
  __shared__ float valb[NE];
  __shared__ double md[NORM ? 2 * OD : 1];                                // entry statistics: mean | 1 / sqrt(var + eps)
  __shared__ float wl[LAG ? (2 * NROT + 2) * NE : 1];                     // rotor states | dynamics factors, [2 NROT + 2][NE]: each lane reads and writes its own column
  constexpr bool kNoiseLds = NOISE && NORM;
  constexpr bool kFailLds = kFail && NORM;                                   // rotor failure: the NORM forms keep the lanes' plans in LDS
  __shared__ int32_t fkl[kFailLds ? 2 * NE : 1];                          // [2][NE] words: key, f; each lane reads and writes its own column
  __shared__ float zl[kNoiseLds ? 13 * NE : 1];                           // sensor noise: the perturbed copy of the 13 state numbers, [13][NE]
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  const int lane = int(threadIdx.x) & 63;
  if constexpr (NORM) {
    for (int j = int(threadIdx.x); j < OD; j += int(blockDim.x)) { md[j] = N.buf[j]; md[OD + j] = 1.0 / sqrt(N.buf[OD + j] + N.eps); }
    __syncthreads();
  }
  if (wave < 4) { policy_mlp_waves<NE, true, 4, false>(io, wave, lane, n_steps, xin, xlo, h1, h2, meanb, valb, nullptr); return; }
  // ---- env wavefronts: one lane per env (NE = 16: lanes 0..15; the others only pass the barriers)
  const int el = (wave - 4) * 64 + lane;                          // env within the workgroup
  const bool mine = NE >= 64 || el < NE;
  const int i = int(blockIdx.x) * NE + (mine ? el : 0);
  const int tl = i & 63;                                          // the env's slot in its 64-env tile
  const bool active = mine && i < n_envs;
  const size_t n = size_t(n_envs);
  char* tile = static_cast<char*>(blob) + size_t(i >> 6) * tile_bytes;
  const int K = KW == 1 ? 1 : P.K;
  Env<float, KW> e;
  DynFac<float, NROT, DR> df;
  FailLane fl{-1, 0.0f};                                          // rotor failure: the episode's plan, spent when the factor holds it
  float std_a[AD], ls_a[AD];
  float o[kObsDimMax];
  double s1[NORM ? OD : 1], s2[NORM ? OD : 1];                    // fp64 column sums / sums of squares of this lane's raw rows 1..T
#pragma unroll
  for (int j = 0; j < (NORM ? OD : 1); j++) { s1[j] = 0.0; s2[j] = 0.0; }
  const bool count = NORM && active && N.update != 0;
  constexpr bool kHist = DELAY && !NORM;                          // the action history is not built into the normaliser forms
  std::conditional_t<kHist, HistRows, NoHist> hr;                 // the given rows that end every published row, row pitch OD + 4 n
  int W = OD;
  if constexpr (kHist) { hr.n = DA.D.hist; hr.hover(); W = OD + 4 * hr.n; }
  auto publish_obs = [&](float* grow, bool add) {                 // observation row -> rollout buffer and (two bf16 parts) the MLP input tile
    float v[OD];
#pragma unroll
    for (int j = 0; j < OD; j++) {
      if constexpr (NORM) {   // obsnorm_apply_kernel's arithmetic
        float x = float((double(o[j]) - md[j]) * md[OD + j]);
        v[j] = x < -N.clip ? -N.clip : (x > N.clip ? N.clip : x);
        if (add) { const double r = double(o[j]); s1[j] += r; s2[j] += r * r; }
      } else {
        v[j] = o[j];
      }
    }
    if (active) store_row<OD>(grow, v);
    __bf16* xr = xin + el * kXS;
    __bf16* xl = xlo + el * kXS;
#pragma unroll
    for (int j = 0; j < OD; j++) { const __bf16 hi = (__bf16)v[j]; xr[j] = hi; xl[j] = (__bf16)(v[j] - float(hi)); }
    if constexpr (kHist) {   // columns OD .. W: raw, neither perturbed nor scaled; two bf16 parts like the others
      if (active) hist_put<OD % 4 == 0>(grow + OD, hr);
      const float g[8] = {hr.g0.x, hr.g0.y, hr.g0.z, hr.g0.w, hr.g1.x, hr.g1.y, hr.g1.z, hr.g1.w};
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (j < 4 * hr.n) { const __bf16 hi = (__bf16)g[j]; xr[OD + j] = hi; xl[OD + j] = (__bf16)(g[j] - float(hi)); }
    }
  };
  if (mine) {
    load_env<float, KW, 0>(K, tile, tl, e);
    if constexpr (DR && !LAG) df = dr_factors<float, NROT, kOwnKey>(P, C, DA.R.r, C.gid0 + i, e.episode);
    if constexpr (LAG) {
#pragma unroll
      for (int r = 0; r < NROT; r++) wl[r * NE + el] = DA.L.w[lag_slot<NROT>(i) + r * 64];
      LagLds<NROT, NE, true>{wl + el, 0.0f, 0.0f}.put(dr_factors<float, NROT, kOwnKey>(P, C, DA.R.r, C.gid0 + i, e.episode));
    }
    if constexpr (kFail) {
      if (DA.R.x.ctl != 0u) fl = fail_draw<NROT>(C, DA.R.x, C.gid0 + i, e.episode);
      if constexpr (kFailLds) fail_put<NE>(fkl + el, fl);
    }
    const uint4* ac = io.pack + size_t(4) * (kPolFrags + kPolBias) * 64;   // policy_pack_kernel's per-entry {std, log_std}
#pragma unroll
    for (int c = 0; c < AD; c++) { const uint4 v = ac[c]; std_a[c] = __uint_as_float(v.x); ls_a[c] = __uint_as_float(v.y); }
    if constexpr (NOISE) {   // row 0: the stored (episode, step) is the key of the row the previous launch (or the reset) published
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
    if constexpr (kHist) {   // row 0 ends in the env's current history
      const int head = (delay_word(DA.D)[i] >> 4) & 7;
      const float4* p = DA.D.h + delay_slot(i);
      if (hr.n > 0) hr.g0 = p[64 * ((head - 1) & 7)];
      if (hr.n > 1) hr.g1 = p[64 * ((head - 2) & 7)];
    }
    publish_obs(io.obs + size_t(i) * W, false);
  }
  const int64_t gid = C.gid0 + i;
  const uint32_t g_lo = uint32_t(uint64_t(gid)), g_hi = uint32_t(uint64_t(gid) >> 32);
  bool any_reset = false;
  StepIO sio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stats};
  const ArmArg<float, 0> AA{0};
  for (int t = 0; t < n_steps; t++) {
    __syncthreads();   // (B0) observation tile published
    __syncthreads();   // (B1)
    __syncthreads();   // (B2)
    __syncthreads();   // (B3)
    __syncthreads();   // (B4) action means and value of this lane's env are in LDS
    if (!mine) continue;
    const float4 m = *reinterpret_cast<const float4*>(meanb + el * 4);
    const float mean[4] = {m.x, m.y, m.z, m.w};
    const float value = valb[el];
    // ---- sample: raw = mean + std z, logp, clip; Philox block 0
    float z[4];
    policy_normal4(io, g_lo, g_hi, io.draw0 + uint32_t(t), 0u, z);
    float act[AD], raw[AD], lp[AD];
#pragma unroll
    for (int c = 0; c < AD; c++) {
      raw[c] = fma_(std_a[c], z[c], mean[c]);
      lp[c] = fma_(-0.5f * z[c], z[c], -ls_a[c]) - kHalfLog2Pi;
      act[c] = policy_clip(raw[c], c);
    }
    const float logp = (lp[0] + lp[1]) + (lp[2] + lp[3]);       // (the quad form's sum4 association)
    const size_t tn = size_t(t) * n;
    if (active) {
      *reinterpret_cast<float4*>(io.actions + (tn + i) * AD) = make_float4(raw[0], raw[1], raw[2], raw[3]);
      io.logp[tn + i] = logp; io.values[tn + i] = value;
    }
    DelayLane dl; float4 given;
    if constexpr (DELAY) {
      given = make_float4(act[0], act[1], act[2], act[3]);
      if constexpr (kHist) { hr.g0 = given; delay_apply(DA.D, i, dl, act, hr); } else delay_apply(DA.D, i, dl, act);
    }
    if constexpr (DR) rate_apply(P, DA.R.q, e, act);   // body-rate actions: behind the clipped action and the latency, in front of the step
    if constexpr (kFailLds) fail_hit_lds<NROT, NE>(fkl + el, e.step, LAG ? nullptr : df.s, wl + el);   // rotor failure: the step field as this step finds it
    else if constexpr (kFail && LAG) fail_hit_scol<NROT, NE>(fl, e.step, wl + el);
    else if constexpr (kFail) fail_hit<float, NROT>(fl, e.step, df.s);
    // ---- env step (amenv_step's lane kernel code); the terminal row is written raw by step_lane and normalised in place below
    sio.terminal_obs = io.terminal_obs ? io.terminal_obs + tn * W : nullptr;
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
    if constexpr (DR && !LAG) { if (was_reset) df = dr_factors<float, NROT, kOwnKey>(P, C, DA.R.r, gid, e.episode); }   // the new episode's vehicle
    if constexpr (LAG) {
      if (was_reset) {   // the new episode's rotors: w0 (behind the states in the side buffer), and the new episode's vehicle
#pragma unroll
        for (int r = 0; r < NROT; r++) wl[r * NE + el] = DA.L.w[size_t(NROT) * DA.L.n_pad + r];
        lg.put(dr_factors<float, NROT, kOwnKey>(P, C, DA.R.r, gid, e.episode));
      }
    }
    if constexpr (kFail) {
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
    accumulate_stats(stats, int(blockIdx.x) * EW + (wave - 4), bits, is_done, ep_len, ep_ret);
    if constexpr (NORM) {
      if (is_done && sio.terminal_obs) {                          // (this lane wrote the row inside step_lane)
        float* tr = sio.terminal_obs + size_t(i) * OD;
#pragma unroll
        for (int j = 0; j < OD; j++) {
          const float x = float((double(tr[j]) - md[j]) * md[OD + j]);
          tr[j] = x < -N.clip ? -N.clip : (x > N.clip ? N.clip : x);
        }
      }
    }
    if (active) {
      io.rewards[tn + i] = reward;
      io.dones[tn + i] = is_done ? 1 : 0;
      if (io.info) io.info[tn + i] = bits;
    }
    publish_obs(io.obs + (tn + n + i) * W, count);              // row t + 1, and the next step's MLP input
  }
  if (mine) {
    store_env_step<float, KW, 0>(tile, tl, e, K);
    if (any_reset) store_env_episode<float, KW>(K, tile, tl, e);
    if constexpr (LAG) {
#pragma unroll
      for (int r = 0; r < NROT; r++) DA.L.w[lag_slot<NROT>(i) + r * 64] = wl[r * NE + el];
    }
  }
  if constexpr (NORM) {
    if (N.update != 0) {   // one reduction per env wavefront (lanes without an active env hold zeros), one atomic per column and wavefront
#pragma unroll
      for (int j = 0; j < OD; j++) {
        double a = s1[j], b = s2[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
        if (lane == 0) { atomicAdd(N.buf + 2 * OD + 1 + j, a); atomicAdd(N.buf + 3 * OD + 1 + j, b); }
      }
    }
  }
}

}  // namespace amenv_dev
