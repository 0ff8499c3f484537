// amenv_lane_policy.hpp -- the closed-loop rollout of amenv_team_policy.hpp for LARGE batches (amenv_rollout_policy above the lane-team
// kernel's range): observation -> actor / critic MLPs -> Gaussian sample -> clip -> env step, T times in one launch, with ONE LANE PER ENV
// for the environment.  The lane-team form spends 16 lanes on an env to be short; from ~8192 envs on every SIMD holds several of its
// wavefronts and the step is bound by their vector-ALU work (~360 wave-instructions per env-step against ~60 for a lane that owns an env).
//   * a workgroup = EW x 64 envs (EW = 1 or 2 env wavefronts, 320 or 384 threads): wavefronts 4.. integrate them (the lane kernel's
//     step_lane: same arithmetic as amenv_step's lane / helper kernels, bit for bit), wavefronts 0..3 run the two MLPs over the workgroup's
//     4 EW column tiles of 16 envs (amenv_policy_mlp.hpp's policy_mlp_waves, single-part first layer: the team kernel's network).  The env
//     code needs ~210 registers, so a SIMD holds two wavefronts and a CU one workgroup: EW = 2 covers 32768 envs with one wave of workgroups
//     on the 256 CUs;
//   * the two halves alternate: five workgroup barriers per step, activations / action means / values through LDS;
//   * the action noise is policy_normal4's (block 0 -> wrench entries, block 1 -> joints: the team kernel's mapping), the log-probability is
//     summed in the team kernel's order: for the same observation both kernels produce the same action, bit for bit;
//   * KW = 1 (one waypoint) or AMENV_MAX_WAYPOINTS (2..4), any joint axes (step_lane branches on them);
//   * PNJ = the caller's joints.  A 1- or 2-link arm runs, inside, the 3-joint vehicle with phantom links (amenv_create pad_arm_config),
//     exactly as amenv_step does; the kernel publishes the CALLER's rows: obs / terminal_obs 23 + 2 PNJ wide in arm_cut_obs_kernel's
//     column order, actions 4 + PNJ wide.  The MLP keeps its 29-wide input tile and 7-row head: policy_pack_kernel gives the phantom
//     inputs and rows zero weights, the phantom joint commands are 0.0f (as arm_pad_actions_kernel pads them) and the log-probability
//     sums the 4 + PNJ real entries.  A terminal row is written 29 wide by step_lane into a per-env staging row (term29) and cut by
//     the lane that wrote it.
#pragma once
#include "amenv_kernels.hpp"
#include "amenv_policy_mlp.hpp"

namespace amenv_dev {

// column of the internal 29-wide row that feeds column j of the caller's row (arm_cut_obs_kernel's map)
template <int PNJ>
__device__ constexpr int arm_pub_src(int j) { return j < 20 + PNJ ? j : (j < 20 + 2 * PNJ ? 23 + (j - 20 - PNJ) : 26 + (j - 20 - 2 * PNJ)); }

template <int NROT, int EW, int KW, int PNJ>
__global__ __launch_bounds__(256 + 64 * EW) void rollout_policy_kernel_lane(void* __restrict__ blob, uint32_t tile_bytes, int32_t n_envs, int n_steps, const PolicyIO io,
                                                                  unsigned long long* __restrict__ stats, const HotParams<float, NROT> P, const ColdParams C,
                                                                  const ArmArg<float, 3> AA, float* __restrict__ term29) {
  constexpr int OD = 29, AD = 7, NE = 64 * EW, NJ = 3;   // envs per workgroup (4 EW column tiles of 16)
  constexpr int POD = 23 + 2 * PNJ, PAD = 4 + PNJ;                      // the caller's row widths
  static_assert(PNJ >= 1 && PNJ <= 3, "1..3 public joints");
  __shared__ __attribute__((aligned(16))) __bf16 xin[NE * kXS];
  __shared__ __attribute__((aligned(16))) __bf16 h1[2 * NE * kH1S];       // layer-1 activations; layer 3's reuse the front of it (h1 is dead by then)
  __shared__ __attribute__((aligned(16))) __bf16 h2[2 * NE * kH2S];
  __shared__ __attribute__((aligned(16))) float meanb[NE * 8];
  __shared__ float valb[NE];
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  const int lane = int(threadIdx.x) & 63;
  if (wave < 4) { policy_mlp_waves<NE, false, 8, false>(io, wave, lane, n_steps, xin, nullptr, h1, h2, meanb, valb, nullptr); return; }
  // ---- env wavefronts: one lane per env
  const int el = (wave - 4) * 64 + lane;                          // env within the workgroup
  const int i = int(blockIdx.x) * NE + el;
  const bool active = i < n_envs;
  const size_t n = size_t(n_envs);
  char* tile = static_cast<char*>(blob) + size_t(i >> 6) * tile_bytes;
  const int K = KW == 1 ? 1 : P.K;
  Env<float, KW> e;
  load_env<float, KW, NJ>(K, tile, lane, e);
  // per-entry action constants (policy_pack_kernel's last block: lanes 0..3 hold entry c of the wrench and joint min(c, 2))
  float std_a[AD], ls_a[AD];
  {
    const uint4* ac = io.pack + size_t(4) * (kPolFrags + kPolBias) * 64;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint4 v = ac[c];
      std_a[c] = __uint_as_float(v.x); ls_a[c] = __uint_as_float(v.y);
      if (c < PNJ) { std_a[4 + c] = __uint_as_float(v.z); ls_a[4 + c] = __uint_as_float(v.w); }
    }
  }
  const int64_t gid = C.gid0 + i;
  const uint32_t g_lo = uint32_t(uint64_t(gid)), g_hi = uint32_t(uint64_t(gid) >> 32);
  const bool ee_task = P.ee_task != 0;
  float o[kObsDimMax];
  update_tool_offset<float, KW, false>(AA.p, e);
  observe<float, KW, true>(K, e, o, ee_task);
  observe_joints<float, KW>(e, o);
  auto publish_obs = [&](float* grow) {                          // observation row -> rollout buffer (the caller's columns) and (bf16) the MLP's input tile
    if (active) {
#pragma unroll
      for (int j = 0; j < POD; j++) grow[j] = o[arm_pub_src<PNJ>(j)];
    }
    __bf16* xr = xin + el * kXS;
#pragma unroll
    for (int j = 0; j < OD; j++) xr[j] = (__bf16)o[j];
  };
  { __bf16* xr = xin + el * kXS; xr[OD] = (__bf16)1.0f; xr[OD + 1] = (__bf16)0.0f; xr[OD + 2] = (__bf16)0.0f; }   // bias column, K padding
  publish_obs(io.obs + size_t(i) * POD);
  bool any_reset = false;
  StepIO sio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stats};
  for (int t = 0; t < n_steps; t++) {
    __syncthreads();   // (B0) observation tile published
    __syncthreads();   // (B1)
    __syncthreads();   // (B2)
    __syncthreads();   // (B3)
    __syncthreads();   // (B4) action means and value of this lane's env are in LDS
    float mean[8];
    {
      const float4 m0 = *reinterpret_cast<const float4*>(meanb + el * 8), m1 = *reinterpret_cast<const float4*>(meanb + el * 8 + 4);
      mean[0] = m0.x; mean[1] = m0.y; mean[2] = m0.z; mean[3] = m0.w; mean[4] = m1.x; mean[5] = m1.y; mean[6] = m1.z; mean[7] = m1.w;
    }
    const float value = valb[el];
    // ---- sample: raw = mean + std z, logp, clip (DiagGaussianDistribution + collect_rollouts' clip); Philox block 0 -> wrench entries, 1 -> joints
    float z[8];
    policy_normal4(io, g_lo, g_hi, io.draw0 + uint32_t(t), 0u, z);
    policy_normal4(io, g_lo, g_hi, io.draw0 + uint32_t(t), 1u, z + 4);
    float act[AD], raw[AD], lp[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      raw[c] = fma_(std_a[c], z[c], mean[c]);
      lp[c] = fma_(-0.5f * z[c], z[c], -ls_a[c]) - kHalfLog2Pi;
      act[c] = policy_clip(raw[c], c);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c < PNJ) {
        raw[4 + c] = fma_(std_a[4 + c], z[4 + c], mean[4 + c]);
        lp[c] = lp[c] + (fma_(-0.5f * z[4 + c], z[4 + c], -ls_a[4 + c]) - kHalfLog2Pi);
        act[4 + c] = clamp_(raw[4 + c], -1.0f, 1.0f);
      } else {
        act[4 + c] = 0.0f;                                        // a phantom joint: no command
      }
    }
    const float logp = (lp[0] + lp[1]) + (lp[2] + lp[3]);       // (the team kernel's quad sum, same association)
    const size_t tn = size_t(t) * n;
    if (active) {
      float* ar = io.actions + (tn + i) * PAD;
#pragma unroll
      for (int c = 0; c < PAD; c++) ar[c] = raw[c];
      io.logp[tn + i] = logp; io.values[tn + i] = value;
    }
    // ---- env step (amenv_step's lane kernel code); a shorter arm's terminal row goes 29 wide to its staging row, then cut below
    sio.terminal_obs = io.terminal_obs ? (PNJ == 3 ? io.terminal_obs + tn * OD : term29) : nullptr;
    float reward; bool was_reset; int ep_len; float ep_ret;
    uint32_t bits;
    if constexpr (KW == 1) {
      bits = step_lane<float, NROT, KW, VAR_V2, NJ>(P, C, AA, e, act, i, active, reward, o, sio, tile, lane, any_reset, was_reset, ep_len, ep_ret);
    } else {   // K made opaque per step: the reset path's waypoint fractions k / K stay in it instead of being hoisted out of the loop and
      HotParams<float, NROT> Pk = P;   // held in registers for the whole rollout (which spills)
      int k = Pk.K;
      asm volatile("" : "+s"(k));
      Pk.K = k;
      bits = step_lane<float, NROT, KW, VAR_V2, NJ>(Pk, C, AA, e, act, i, active, reward, o, sio, tile, lane, any_reset, was_reset, ep_len, ep_ret);
    }
    any_reset |= was_reset;
    const bool is_done = active && (bits & (AMENV_INFO_TERMINATED | AMENV_INFO_TRUNCATED)) != 0;
    accumulate_stats(stats, int(blockIdx.x) * EW + (wave - 4), bits, is_done, ep_len, ep_ret);
    if constexpr (PNJ < 3) {
      if (is_done && sio.terminal_obs) {                          // (this lane wrote the staging row inside step_lane)
        const float* src = term29 + size_t(i) * OD;
        float* dst = io.terminal_obs + (tn + i) * POD;
#pragma unroll
        for (int j = 0; j < POD; j++) dst[j] = src[arm_pub_src<PNJ>(j)];
      }
    }
    if (active) {
      io.rewards[tn + i] = reward;
      io.dones[tn + i] = is_done ? 1 : 0;
      if (io.info) io.info[tn + i] = bits;
    }
    publish_obs(io.obs + (tn + n + i) * POD);                    // row t + 1, and the next step's MLP input
  }
  if constexpr (KW > 1) asm volatile("" : "+v"(tile));          // (the joint groups' addresses are formed here, not kept from the load)
  store_env_step<float, KW, NJ>(tile, lane, e, K);
  if (any_reset) store_env_episode<float, KW>(K, tile, lane, e);
}

}  // namespace amenv_dev
