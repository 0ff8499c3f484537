// amenv_policy_mlp.hpp -- the actor / critic network of the one-launch closed loops (rollout_policy_kernel_*, evaluate_policy_kernel_*): SB3's
// MlpPolicy [128, 64, 64] tanh with separate actor / critic trunks (v2/rl_train.py:38-56), its packed form, the forward pass of the wave-split
// kernels and the action sampler.  THE description of the MLP part; the kernels' headers point here.
//   * the two MLPs run on the matrix cores in bf16 with fp32 accumulation (v_mfma_f32_16x16x32_bf16): this IS a dense contraction --
//     north_star's "no MFMA" is about step().  Orientation D = W . X^T: M = 16 output neurons, N = a column tile of 16 envs, K = inputs, so a
//     lane ends up with 4 consecutive neurons of one env (one 8-byte LDS store) and the next layer's B operand is 8 consecutive inputs of one
//     env (one 16-byte LDS load).  Per step and 16-env tile: 18 MFMAs per wavefront (22 with the two-part first layer);
//   * four wavefronts share the neurons: layer 1 is 4 of the 16 tiles of the combined [actor | critic] 256 neurons each; in layers 2 and 3
//     wavefronts 0, 1 hold the actor and 2, 3 the critic; wavefront 0 computes the action means and wavefront 1 the value.  The weights are
//     loop-invariant A operands: each wavefront keeps its 18 fragments (72 VGPRs) and 5 bias quadruples in registers for the whole launch
//     (policy_pack_kernel lays them out in that order) -- no weight traffic per step;
//   * activations travel through LDS (bf16), 5 workgroup barriers per step (B0..B4 in policy_mlp_waves); tanh = 1 - 2 / (exp(2x) + 1) on v_exp / v_rcp;
//   * the rigid vehicles' first layer takes the observation and its weights as TWO bf16 parts each (x = hi + lo to ~2^-17 relative): a trained
//     controller's first layer amplifies the 2^-9 rounding of a single bf16 input to ~0.1 in the action (measured on the reference checkpoint,
//     0.03 with the input split), so three products hi.hi + hi.lo + lo.hi per tile give the first layer ~fp32 accuracy for two more
//     MFMAs.  The residual fragments sit behind the action constants (kPolLoBase);
//   * action noise: Philox4x32-10 keyed (seed, global env id, draw index, block) as amenv_gaussian_act, Box-Muller on the fast intrinsics
//     (v_log / v_sin / v_cos): the same distribution, not the same bits as the one-launch-per-op path.  Block 0 = the four wrench entries,
//     block 1 = the joints; pairs (w0, w1) -> entries 0 (cos), 1 (sin), (w2, w3) -> entries 2, 3.
// bf16 rounding perturbs the action means by ~1e-2 of their scale: an opt-in ROLLOUT mode (ppo.py fused_rollout=True); parity paths keep amenv_policy.hpp.
// rollout_policy_kernel_team / _quad run the same layers on wavefronts that also hold env state in registers and keep their own copy.
#pragma once
#include "amenv_model.hpp"

namespace amenv_dev {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPolFrags = 18, kPolBias = 5;                  // per wavefront: weight fragments (uint4 per lane), bias quadruples (float4 per lane)
constexpr int kPolLoBase = (4 * (kPolFrags + kPolBias) + 1) * 64;          // uint4 index of the first-layer residual fragments (rigid-vehicle rollout)
constexpr int kPolPackWords = (kPolLoBase + 4 * 4 * 64) * 4;                // dwords of the packed policy: 4 wavefronts + one block of action constants + W1 residuals
constexpr int kXS = 40, kH1S = 136, kH2S = 72;               // LDS row strides (bf16 elements): 32 / 128 / 64 + 8 of padding
constexpr float kHalfLog2Pi = 0.918938533204672742f;         // the Gaussian log-density's constant, per action entry

// the action box (v2/rl_env_scaledObs.py): entry 0 (thrust) in [0, 2], every other entry in [-1, 1]
__device__ __forceinline__ constexpr float policy_box_lo(int c) { return c == 0 ? 0.0f : -1.0f; }
__device__ __forceinline__ constexpr float policy_box_hi(int c) { return c == 0 ? 2.0f : 1.0f; }
__device__ __forceinline__ float policy_clip(float x, int c) { return clamp_(x, policy_box_lo(c), policy_box_hi(c)); }

// Flat parameter buffer (SB3 state-dict order, ppo.py ActorCritic.flatten_):
//   log_std[A] | pi.0 W[128,D] b | pi.2 W[64,128] b | pi.4 W[64,64] b | vf.0 .. vf.4 (same shapes) | action W[A,64] b | value W[1,64] b
struct PolLayout {
  int D, A, trunk, o_pi, o_vf, o_actw, o_actb, o_valw, o_valb;
  __host__ __device__ PolLayout(int d, int a) : D(d), A(a) {
    trunk = 128 * D + 128 + 64 * 128 + 64 + 64 * 64 + 64;
    o_pi = A; o_vf = o_pi + trunk; o_actw = o_vf + trunk; o_actb = o_actw + A * 64; o_valw = o_actb + A; o_valb = o_valw + 64;
  }
};

__device__ __forceinline__ uint32_t bf16_bits(float x) { return uint32_t(__builtin_bit_cast(unsigned short, (__bf16)x)); }

// Column of the caller's observation row that feeds input k of the first layer (k == the tile's width: the bias column), -1: a zero
// weight.  pnj = 0: the caller's row IS the tile (D inputs).  pnj = 1, 2: a 1- / 2-link arm whose env runs the 3-joint vehicle: the
// tile is the internal 29-wide row (20 | th(3) | thd(3) | tool(3)) and the caller's the 23 + 2 pnj of arm_cut_obs_kernel; the phantom
// links' th / thd inputs get zero weights, so the MLP depends on the caller's columns only.
__device__ __forceinline__ int pol_in_col(int k, int D, int pnj) {
  if (pnj == 0) return k <= D ? k : -1;
  if (k < 20) return k;
  if (k < 23) return k - 20 < pnj ? k : -1;
  if (k < 26) return k - 23 < pnj ? 20 + pnj + (k - 23) : -1;
  if (k < 29) return 20 + 2 * pnj + (k - 26);
  return k == 29 ? D : -1;
}
__device__ __forceinline__ float pol_w1(const float* W1, const float* b1, int neuron, int k, int D, int pnj) {
  const int c = pol_in_col(k, D, pnj);
  return c < 0 ? 0.0f : (c < D ? W1[neuron * D + c] : b1[neuron]);
}

// (policy_pack_kernel, which writes the packed form: amenv_policy_pack.hpp)

struct PolicyIO {
  const uint4* pack;        // policy_pack_kernel output
  uint32_t seed_lo, seed_hi, draw0;
  float* obs;               // [T + 1][N][29]: row 0 = observation of the state at entry, row t + 1 = after step t
  float* actions;           // [T][N][7]  raw (unclipped) samples, as SB3's rollout buffer stores them
  float* logp;              // [T][N]
  float* values;            // [T][N]
  float* rewards;           // [T][N]
  uint8_t* dones;           // [T][N]
  uint32_t* info;           // [T][N] or null
  float* terminal_obs;      // [T][N][29] or null: rows written only where the episode ended at step t
};

__device__ __forceinline__ float fast_tanh(float x) {   // 1 - 2 / (exp(2x) + 1): exact limits, ~1e-6 abs elsewhere
  const float t = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f);
}

// THE EXIT PROTOCOL (the evaluation kernels, EXIT below).  `pend` is one LDS word with ONE writer, lane 0 of the workgroup's only env wavefront:
//   (w0) before its barrier B0 of step 0 it writes "an env of this workgroup is short of its quota";
//   (w)  after its barrier B4 of step t it writes the same for the state after step t.
// EVERY wavefront (the four MLP ones here, the env one through eval_pending) reads `pend` directly behind B0 of step t and leaves the loop when it is 0.
// Why all five read the same value: the write (w) of step t - 1 (or (w0)) precedes the writer's arrival at B0(t), so it is visible behind B0(t) to
// all; the NEXT write happens behind the writer's B4(t), which it passes only after every wavefront has arrived at B1(t) .. B4(t), and a wavefront
// arrives at B1(t) only after it has branched on the value read behind B0(t) (the read has returned by then).  So no read of
// step t can see the write of step t, all five wavefronts take the same decision in the same iteration, and each has executed exactly 5 t barriers
// when it leaves: none is left waiting.  max_steps bounds the loop for all alike (a kernel argument).  No barrier follows the loop.
__device__ __forceinline__ bool eval_pending(const int* pend) { return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const volatile int*>(pend)) != 0; }

// The MLP wavefronts' half of the WAVE-SPLIT kernels (wavefronts 0..3 the MLPs, 4.. the envs: rollout_policy_kernel_rigid / _lane and the two
// evaluate_policy_kernel_*): wavefront `wave` computes its neuron subset for the workgroup's NE envs (NE / 16 column tiles), max_steps times.
// Per step, between the barriers the env wavefronts pass as well:
//   (B0) the observation tile xin (LO: and its second part xlo) is complete      -> layer 1 -> h1
//   (B1)                                                                         -> layer 2 -> h2
//   (B2) h1 has been read by everyone: layer 3 overwrites its front              -> layer 3 -> h1
//   (B3)                                                                         -> heads  -> meanb (MW floats per env), valb
//   (B4) means and values are there: the env wavefronts sample, step and publish the next tile
// LO: the two-part first layer (the rigid vehicles); MW: the mean row's width, 4 (rigid) or 8 (arm); EXIT: leave behind B0 when `pend` is 0.
template <int NE, bool LO, int MW, bool EXIT>
__device__ __forceinline__ void policy_mlp_waves(const PolicyIO& io, int wave, int lane, int max_steps, const __bf16* xin, const __bf16* xlo, __bf16* h1, __bf16* h2,
                                                 float* meanb, float* valb, const int* pend) {
  constexpr int NT = NE / 16;
  __bf16* h3 = h1;
  uint4 wf[kPolFrags], wlo[LO ? 4 : 1];
  f32x4 bias[kPolBias];
  if constexpr (LO) {
#pragma unroll
    for (int k = 0; k < 4; k++) wlo[k] = io.pack[size_t(kPolLoBase) + size_t(4 * wave + k) * 64 + lane];
  }
  {
    const uint4* src = io.pack + size_t(wave) * (kPolFrags + kPolBias) * 64 + lane;
#pragma unroll
    for (int k = 0; k < kPolFrags; k++) wf[k] = src[k * 64];
#pragma unroll
    for (int k = 0; k < kPolBias; k++) { const uint4 b = src[(kPolFrags + k) * 64]; bias[k] = f32x4{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)}; }
  }
  const int nrow = lane & 15, kq = lane >> 4;
  auto load_b = [&](const __bf16* base, int stride, int et, int ks) {   // operand B: 8 consecutive inputs of env 16 et + nrow
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(base + (16 * et + nrow) * stride + 32 * ks + 8 * kq));
  };
  auto store_d = [&](__bf16* base, int stride, int et, int tile16, const f32x4& acc) {   // tanh, 4 consecutive neurons of that env
    const f32x4 t{fast_tanh(acc[0]), fast_tanh(acc[1]), fast_tanh(acc[2]), fast_tanh(acc[3])};
    *reinterpret_cast<uint2*>(base + (16 * et + nrow) * stride + 16 * tile16 + 4 * kq) = __builtin_bit_cast(uint2, __builtin_convertvector(t, bf16x4));
  };
  const int net23 = wave >> 1;                                  // layers 2, 3: wavefronts 0, 1 the actor, 2, 3 the critic
  for (int t = 0; t < max_steps; t++) {
    __syncthreads();                                            // (B0) the observation tile is complete
    if constexpr (EXIT) { if (!eval_pending(pend)) break; }     // (the exit protocol above: the env wavefront leaves in this iteration too)
#pragma unroll
    for (int et = 0; et < NT; et++) {                            // layer 1, K = 32 (LO: hi.hi + hi.lo + lo.hi)
      const bf16x8 B = load_b(xin, kXS, et, 0);
      bf16x8 Bl;
      if constexpr (LO) Bl = load_b(xlo, kXS, et, 0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int T = 4 * wave + j, net = T >> 3;
        f32x4 acc{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (LO) {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wlo[j]), B, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[j]), Bl, acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[j]), B, acc, 0, 0, 0);
        store_d(h1 + net * NE * kH1S, kH1S, et, T & 7, acc);
      }
    }
    __syncthreads();                                            // (B1)
#pragma unroll
    for (int et = 0; et < NT; et++) {
      bf16x8 B[4];
#pragma unroll
      for (int ks = 0; ks < 4; ks++) B[ks] = load_b(h1 + net23 * NE * kH1S, kH1S, et, ks);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        f32x4 acc = bias[j];
#pragma unroll
        for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[4 + 4 * j + ks]), B[ks], acc, 0, 0, 0);
        store_d(h2 + net23 * NE * kH2S, kH2S, et, (2 * wave + j) & 3, acc);
      }
    }
    __syncthreads();                                            // (B2) h1 has been read by everyone: layer 3 may overwrite it
#pragma unroll
    for (int et = 0; et < NT; et++) {
      bf16x8 B[2];
#pragma unroll
      for (int ks = 0; ks < 2; ks++) B[ks] = load_b(h2 + net23 * NE * kH2S, kH2S, et, ks);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        f32x4 acc = bias[2 + j];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[12 + 2 * j + ks]), B[ks], acc, 0, 0, 0);
        store_d(h3 + net23 * NE * kH2S, kH2S, et, (2 * wave + j) & 3, acc);
      }
    }
    __syncthreads();                                            // (B3)
    if (wave < 2) {   // heads: wavefront 0 the action mean, wavefront 1 the value (row 0)
#pragma unroll
      for (int et = 0; et < NT; et++) {
        f32x4 acc = bias[4];
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[16 + ks]), load_b(h3 + wave * NE * kH2S, kH2S, et, ks), acc, 0, 0, 0);
        if (wave == 0) { if (kq < MW / 4) *reinterpret_cast<float4*>(meanb + (16 * et + nrow) * MW + 4 * kq) = make_float4(acc[0], acc[1], acc[2], acc[3]); }
        else if (kq == 0) valb[16 * et + nrow] = acc[0];
      }
    }
    __syncthreads();                                            // (B4) means and values are there
  }
}

// the four unit normals of Philox block b for (seed, env, draw): pairs (w0, w1) -> z[0] (cos), z[1] (sin), (w2, w3) -> z[2], z[3]
__device__ __forceinline__ void policy_normal4(const PolicyIO& io, uint32_t g_lo, uint32_t g_hi, uint32_t draw, uint32_t b, float* z) {
  uint32_t w4[4];
  philox4x32_10(io.seed_lo ^ 0x5bd1e995u, io.seed_hi ^ 0x27d4eb2fu, g_lo, g_hi, draw, b, w4);
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const float u1 = float((w4[2 * p] >> 8) + 1u) * 5.9604644775390625e-08f, u2 = float(w4[2 * p + 1] >> 8) * 5.9604644775390625e-08f;
    const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
    const float ang = 6.28318530717958647692f * u2;
    z[2 * p] = rad * __cosf(ang);
    z[2 * p + 1] = rad * __sinf(ang);
  }
}

}  // namespace amenv_dev
