// amenv_team_policy.hpp -- closed-loop rollout in ONE launch: observation -> actor / critic MLPs -> Gaussian sample -> clip -> env step,
// T times, for the hexacopter + arm on the lane-team layout (amenv_team.hpp).  This is the loop SB3's collect_rollouts runs
// (v2/rl_train.py:38-56) with nothing leaving the chip between steps:
//   * a 256-thread workgroup = 4 wavefronts = 16 envs (16 lanes per env); env state and the per-lane constants stay in registers;
//   * the network, its packed weights, the five barriers per step and the sampler's keying: amenv_policy_mlp.hpp.
// The shared forward pass lives there (policy_mlp_waves); this kernel keeps its own copy of the layers: all four wavefronts run the MLP AND hold
// env state in registers (OCC = 2 at 256 registers), so they cannot call a function that owns the step loop.
// Above the lane-team kernel's batch range the same loop runs with one lane per env for the environment: amenv_lane_policy.hpp.
#pragma once
#include "amenv_policy_mlp.hpp"
#include "amenv_team.hpp"

namespace amenv_dev {

// OCC = wavefronts per SIMD the register allocation leaves room for: 1 in the latency regime (one workgroup per CU: all 512 registers,
// no spills), 2 in the throughput regime (<= 256 registers, a few spills, twice the resident wavefronts per SIMD).
template <int NROT, int OCC>
__global__ __launch_bounds__(256, OCC) void rollout_policy_kernel_team(void* __restrict__ blob, uint32_t tile_bytes, int32_t n_envs, int n_steps, const PolicyIO io,
                                                                  unsigned long long* __restrict__ stats, const ColdParams C, const TeamParams P) {
  constexpr int OD = 29, AD = 7;
  __shared__ __attribute__((aligned(16))) __bf16 xin[16 * kXS];
  __shared__ __attribute__((aligned(16))) __bf16 h1[2 * 16 * kH1S];
  __shared__ __attribute__((aligned(16))) __bf16 h2[2 * 16 * kH2S];
  __shared__ __attribute__((aligned(16))) __bf16 h3[2 * 16 * kH2S];
  __shared__ __attribute__((aligned(16))) float meanb[16 * 8];
  __shared__ float valb[16];
  TeamLane L;
  L.init(P);
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  const int el = wave * 4 + (L.lane >> 4);                   // env within the workgroup
  const int i = int(blockIdx.x) * 16 + el;
  const bool active = i < n_envs;
  char* tile = static_cast<char*>(blob) + size_t(i >> 6) * tile_bytes;
  // this wavefront's weight fragments and biases: loop-invariant, in registers
  uint4 wf[kPolFrags];
  f32x4 bias[kPolBias];
  {
    const uint4* src = io.pack + size_t(wave) * (kPolFrags + kPolBias) * 64 + L.lane;
#pragma unroll
    for (int k = 0; k < kPolFrags; k++) wf[k] = src[k * 64];
#pragma unroll
    for (int k = 0; k < kPolBias; k++) { const uint4 b = src[(kPolFrags + k) * 64]; bias[k] = f32x4{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)}; }
  }
  TeamEnv E;
  team_load(tile, i, L, E);
  // per-lane action constants: std / log_std of the wrench entry (lane c) and of the joint (lane c < 3), action box
  const int cj = L.cc < 3 ? L.cc : 2;
  const uint4 ac = io.pack[size_t(4) * (kPolFrags + kPolBias) * 64 + L.lane];
  const float std_w = __uint_as_float(ac.x), ls_w = __uint_as_float(ac.y), std_j = __uint_as_float(ac.z), ls_j = __uint_as_float(ac.w);
  const float lo_w = policy_box_lo(L.cc), hi_w = policy_box_hi(L.cc);
  const int64_t gid = C.gid0 + i;
  const uint32_t g_lo = uint32_t(uint64_t(gid)), g_hi = uint32_t(uint64_t(gid) >> 32);
  const size_t n = size_t(n_envs);
  const int nrow = L.lane & 15, kq = L.lane >> 4;              // MFMA roles of this lane: env column / k-quarter (operand B), neuron quarter (result D)
  // observation of the state at entry -> row 0 of the buffer and the MLP input tile
  float vA, vB, vC;
  team_obs_vals(P, L, E, team_tool_offset(P, L.c, E.y), vA, vB, vC);
  auto publish_obs = [&](float* grow) {
    if (active) {
      if (L.okA) grow[L.offA] = vA;
      if (L.okB) grow[L.offB] = vB;
      if (L.okC) grow[L.offC] = vC;
    }
    __bf16* xr = xin + el * kXS;
    if (L.okA) xr[L.offA] = (__bf16)vA;
    if (L.okB) xr[L.offB] = (__bf16)vB;
    if (L.okC) xr[L.offC] = (__bf16)vC;
  };
  if (L.lead) { __bf16* xr = xin + el * kXS; xr[OD] = (__bf16)1.0f; xr[OD + 1] = (__bf16)0.0f; xr[OD + 2] = (__bf16)0.0f; }   // bias column, K padding
  publish_obs(io.obs + size_t(i) * OD);
  auto load_b = [&](const __bf16* base, int stride, int ks) {   // operand B: 8 consecutive inputs of env `nrow`
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(base + nrow * stride + 32 * ks + 8 * kq));
  };
  auto store_d = [&](__bf16* base, int stride, int tile16, const f32x4& acc) {   // tanh, 4 consecutive neurons of env `nrow`
    const f32x4 t{fast_tanh(acc[0]), fast_tanh(acc[1]), fast_tanh(acc[2]), fast_tanh(acc[3])};
    *reinterpret_cast<uint2*>(base + nrow * stride + 16 * tile16 + 4 * kq) = __builtin_bit_cast(uint2, __builtin_convertvector(t, bf16x4));
  };
  for (int t = 0; t < n_steps; t++) {
    __syncthreads();                                            // the observation tile is complete
    {   // layer 1: 4 tiles of the combined [actor | critic] 256 neurons, K = 32 (29 inputs + bias column)
      const bf16x8 B = load_b(xin, kXS, 0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int T = 4 * wave + j, net = T >> 3;
        f32x4 acc{0.0f, 0.0f, 0.0f, 0.0f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[j]), B, acc, 0, 0, 0);
        store_d(h1 + net * 16 * kH1S, kH1S, T & 7, acc);
      }
    }
    __syncthreads();
    const int net23 = wave >> 1;                                // layers 2, 3: wavefronts 0, 1 the actor, 2, 3 the critic
    {
      bf16x8 B[4];
#pragma unroll
      for (int ks = 0; ks < 4; ks++) B[ks] = load_b(h1 + net23 * 16 * kH1S, kH1S, ks);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        f32x4 acc = bias[j];
#pragma unroll
        for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[4 + 4 * j + ks]), B[ks], acc, 0, 0, 0);
        store_d(h2 + net23 * 16 * kH2S, kH2S, (2 * wave + j) & 3, acc);
      }
    }
    __syncthreads();
    {
      bf16x8 B[2];
#pragma unroll
      for (int ks = 0; ks < 2; ks++) B[ks] = load_b(h2 + net23 * 16 * kH2S, kH2S, ks);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        f32x4 acc = bias[2 + j];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[12 + 2 * j + ks]), B[ks], acc, 0, 0, 0);
        store_d(h3 + net23 * 16 * kH2S, kH2S, (2 * wave + j) & 3, acc);
      }
    }
    __syncthreads();
    if (wave < 2) {   // heads: wavefront 0 the action mean (rows 0..6), wavefront 1 the value (row 0)
      f32x4 acc = bias[4];
#pragma unroll
      for (int ks = 0; ks < 2; ks++)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[16 + ks]), load_b(h3 + wave * 16 * kH2S, kH2S, ks), acc, 0, 0, 0);
      if (wave == 0) { if (kq < 2) *reinterpret_cast<float4*>(meanb + nrow * 8 + 4 * kq) = make_float4(acc[0], acc[1], acc[2], acc[3]); }
      else if (kq == 0) valb[nrow] = acc[0];
    }
    __syncthreads();
    // ---- sample: raw = mean + std z, logp, clip (DiagGaussianDistribution + collect_rollouts' clip).  Even quads draw Philox block 0
    // (wrench entries), odd quads block 1 (joints); the neighbour quad's draws arrive by one DPP row rotation.
    const float mean_w = meanb[el * 8 + L.cc], mean_j = meanb[el * 8 + 4 + cj], value = valb[el];
    float z_mine;
    {
      uint32_t w4[4];
      philox4x32_10(io.seed_lo ^ 0x5bd1e995u, io.seed_hi ^ 0x27d4eb2fu, g_lo, g_hi, io.draw0 + uint32_t(t), uint32_t(L.bb & 1), w4);
      const uint32_t wa = L.cc < 2 ? w4[0] : w4[2], wb = L.cc < 2 ? w4[1] : w4[3];
      const float u1 = float((wa >> 8) + 1u) * 5.9604644775390625e-08f, u2 = float(wb >> 8) * 5.9604644775390625e-08f;
      const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
      const float ang = 6.28318530717958647692f * u2;
      z_mine = rad * ((L.cc & 1) ? __sinf(ang) : __cosf(ang));
    }
    const float z_other = row_ror<4>(z_mine);
    const float zw = (L.bb & 1) ? z_other : z_mine, zj = (L.bb & 1) ? z_mine : z_other;
    const float raw_w = fma_(std_w, zw, mean_w), raw_j = fma_(std_j, zj, mean_j);
    const float lw = fma_(-0.5f * zw, zw, -ls_w) - kHalfLog2Pi;
    const float lj = L.cc < 3 ? fma_(-0.5f * zj, zj, -ls_j) - kHalfLog2Pi : 0.0f;
    const float logp = sum4(lw + lj);
    const float act = clamp_(raw_w, lo_w, hi_w), actj = clamp_(raw_j, -1.0f, 1.0f);
    const size_t tn = size_t(t) * n;
    if (active && L.q0) {
      float* ar = io.actions + (tn + i) * AD;
      ar[L.cc] = raw_w;
      if (L.cc < 3) ar[4 + L.cc] = raw_j;
      if (L.lead) { io.logp[tn + i] = logp; io.values[tn + i] = value; }
    }
    // ---- env step
    const TeamOut o = team_advance<NROT>(P, C, L, E, act, actj, i, active, io.terminal_obs ? io.terminal_obs + tn * OD : nullptr, nullptr, nullptr);
    accumulate_stats(stats, int(blockIdx.x) * 4 + wave, o.bits, active && o.ended && L.lead, o.ep_len, o.ep_ret);
    if (active && L.lead) {
      io.rewards[tn + i] = o.reward;
      io.dones[tn + i] = o.ended ? 1 : 0;
      if (io.info) io.info[tn + i] = o.bits;
    }
    vA = o.vA; vB = o.vB; vC = o.vC;
    publish_obs(io.obs + (tn + n + i) * OD);                   // row t + 1, and the next step's MLP input (xin was last read before the second barrier)
  }
  team_store(tile, i, L, E);
}

}  // namespace amenv_dev
