// amenv_capi_train.hip -- the PPO side of the C ABI: amenv_gae, amenv_gaussian_act, amenv_policy_forward(_mfma) and every amenv_ppo_*.  The one
// source that includes amenv_policy.hpp, amenv_train.hpp and amenv_mlp_train.hpp, whose kernels it alone holds.  DESIGN 4x.
#include "amenv_host.hpp"
#include "amenv_policy.hpp"
#include "amenv_train.hpp"
#include "amenv_mlp_train.hpp"

// workspace of amenv_ppo_mlp_step: advantage partials | split-weight streams of both nets | per-workgroup gradient slabs of both nets
namespace {
constexpr size_t kMlpWsAdv = size_t(2) * kPpoMaxBlocks * sizeof(double);
constexpr size_t kMlpWsWt = size_t(2) * kMlpFragsPerNet * 1024;
constexpr size_t kMlpWsPart = size_t(2) * kMlpMaxBlocks * kAccSize * sizeof(float);
constexpr size_t kMlpLds = kMlpLdsBytes;
template <bool kCtl, int D, int A, bool kVclip = false>   // kVclip: the third form (ctl may be NULL there), with the old values and clip_range_vf
hipError_t launch_mlp_step(const float* Pm, const u32x4* WS, const float* obs, const float* actions, const float* old_logp, const float* adv, const float* ret,
                           const int64_t* index, int64_t n,
                           float clip, float vf, int normalize, const double* adv_part, int adv_blocks, float* part, int blocks, amenv_ppo_ctl* ctl, hipStream_t s,
                           const float* old_values = nullptr, float clip_vf = 0.0f) {
  // > 64 KB of dynamic LDS needs the attribute on the device the launch goes to (the PPO entry points run on the CURRENT device): kept per
  // device, under a lock -- a process that drives several GPUs would otherwise launch without it on the second one
  {
    static std::mutex mu;
    static bool attr_set[64] = {false};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      e = hipFuncSetAttribute(kVclip ? reinterpret_cast<const void*>(&ppo_mlp_fused_kernel_vclip<D, A>)
                              : kCtl ? reinterpret_cast<const void*>(&ppo_mlp_fused_kernel_ctl<D, A>) : reinterpret_cast<const void*>(&ppo_mlp_fused_kernel<D, A>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(kMlpLds));
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  if (kVclip)
    hipLaunchKernelGGL((ppo_mlp_fused_kernel_vclip<D, A>), dim3(blocks, 2), dim3(256), kMlpLds, s, ctl, Pm, WS, obs, actions, old_logp, adv, ret, index, n, clip, vf, normalize,
                       adv_part, adv_blocks, part, old_values, clip_vf);
  else if (kCtl)
    hipLaunchKernelGGL((ppo_mlp_fused_kernel_ctl<D, A>), dim3(blocks, 2), dim3(256), kMlpLds, s, ctl, Pm, WS, obs, actions, old_logp, adv, ret, index, n, clip, vf, normalize,
                       adv_part, adv_blocks, part);
  else
    hipLaunchKernelGGL((ppo_mlp_fused_kernel<D, A>), dim3(blocks, 2), dim3(256), kMlpLds, s, Pm, WS, obs, actions, old_logp, adv, ret, index, n, clip, vf, normalize, adv_part,
                       adv_blocks, part);
  return hipGetLastError();
}
}  // namespace

extern "C" {

// ---- PPO helpers (row f3): GAE over a [T, N] rollout buffer, Gaussian action sampling ------------------------------
int amenv_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values, float* advantages,
              float* returns, int32_t n_steps, int64_t n_envs, float gamma, float gae_lambda, void* stream) {
  if (!rewards || !values || !dones || !last_values || !advantages || !returns || n_steps <= 0 || n_envs <= 0 ||
      !(gamma >= 0.0f && gamma <= 1.0f) || !(gae_lambda >= 0.0f && gae_lambda <= 1.0f))
    return AMENV_ERR_INVALID;
  const int bs = n_envs <= 65536 ? 64 : 256;
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n_envs + bs - 1) / bs)), dim3(bs), 0, (hipStream_t)stream, rewards, values, dones,
                     last_values, advantages, returns, (int)n_steps, (int64_t)n_envs, gamma, gae_lambda);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_gaussian_act(const float* mean, const float* log_std, const float* low, const float* high, float* raw, float* clipped,
                       float* logp, int64_t n_envs, int32_t act_dim, uint64_t seed, uint32_t draw, int64_t env_id_offset, void* stream) {
  if (!mean || !log_std || !low || !high || !raw || !clipped || !logp || n_envs <= 0 || env_id_offset < 0 || !act_dim_built(act_dim)) return AMENV_ERR_INVALID;
  const int bs = n_envs <= 65536 ? 64 : 256;
  const dim3 grid((unsigned)((n_envs + bs - 1) / bs)), block(bs);
  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
  const hipError_t st = with_act_dim(act_dim, [&](auto a) {
    hipLaunchKernelGGL(gaussian_act_kernel<decltype(a)::value>, grid, block, 0, (hipStream_t)stream, mean, log_std, low, high, raw, clipped, logp, (int64_t)n_envs, s_lo, s_hi, draw, (int64_t)env_id_offset);
    return hipGetLastError();
  });
  return st == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_policy_forward(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, int64_t n, float* mean_out,
                         float* value_out, void* stream) {
  if (!flat_params || !obs || n <= 0 || (!mean_out && !value_out) || !policy_shape_built(obs_dim, act_dim)) return AMENV_ERR_INVALID;
  const dim3 grid((unsigned)((n + 63) / 64), 2), block(64 * kPolWaves);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t st = with_policy_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((policy_forward_kernel<decltype(d)::value, decltype(a)::value>), grid, block, 0, s, flat_params, obs, (int64_t)n, mean_out, value_out);
    return hipGetLastError();
  });
  return st == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_policy_forward_mfma(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, int64_t n, float* mean_out, float* value_out,
                              void* workspace, void* stream) {
  if (!flat_params || !obs || n <= 0 || (!mean_out && !value_out) || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || !policy_shape_built(obs_dim, act_dim))
    return AMENV_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  uint16_t* WS = reinterpret_cast<uint16_t*>(static_cast<char*>(workspace) + kMlpWsAdv);   // the split-weight area of amenv_ppo_mlp_step's workspace
  hipLaunchKernelGGL(mlp_pack_kernel, dim3((2 * kMlpPackThreadsPerNet + 255) / 256), dim3(256), 0, s, flat_params, (int)obs_dim, (int)act_dim, WS);
  const int64_t ntiles = (n + 31) / 32;
  const int nets = (mean_out ? 1 : 0) + (value_out ? 1 : 0);   // two wavefronts per SIMD (242 registers): 512 workgroups fill the chip
  const dim3 grid((unsigned)std::min<int64_t>(512 / nets, (ntiles + 3) / 4), 2), block(256);
  const u32x4* ws = reinterpret_cast<const u32x4*>(WS);
  const hipError_t st = with_policy_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((mlp_forward_kernel<decltype(d)::value, decltype(a)::value>), grid, block, 0, s, flat_params, ws, obs, (int64_t)n, mean_out, value_out);
    return hipGetLastError();   // (of the pack kernel's launch too)
  });
  return st == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

size_t amenv_ppo_workspace_bytes(void) { return size_t(kPpoMaxBlocks) * (2 * sizeof(double) + kPpoPartial * sizeof(float)); }

size_t amenv_ppo_ctl_bytes(void) { return sizeof(amenv_ppo_ctl); }

int amenv_ppo_ctl_arm(amenv_ppo_ctl* ctl, float kl_limit, void* stream) {
  if (!ctl || (reinterpret_cast<uintptr_t>(ctl) & 3u) || kl_limit != kl_limit) return AMENV_ERR_INVALID;
  hipLaunchKernelGGL(ppo_ctl_arm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctl, kl_limit);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

// The plain entry point and the _ctl one state their launch geometry themselves and share one launcher; the plain one passes no control
// block.  RULE: the geometry lines of a _ctl entry point are a verbatim copy of its plain twin's -- tests/test_launch_geometry_cpu.py derives
// the thresholds from the plain one's body, and both launch on the same workspace layout: change one, change the other.
static int ppo_loss_grad_launch(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                                const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                                float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats4,
                                void* workspace, amenv_ppo_ctl* ctl, int blocks, void* stream, const float* old_values = nullptr, float clip_range_vf = 0.0f) {
  if (reinterpret_cast<uintptr_t>(ctl) & 3u) return AMENV_ERR_INVALID;
  if (!mean || !value || !log_std || !actions || !old_logp || !advantages || !returns || !d_mean || !d_value || !d_log_std || !stats4 ||
      !workspace || n <= 0 || !(clip_range >= 0.0f) || (reinterpret_cast<uintptr_t>(workspace) & 7u) || !act_dim_built(act_dim))
    return AMENV_ERR_INVALID;
  double* adv_part = static_cast<double*>(workspace);
  float* part = reinterpret_cast<float*>(adv_part + 2 * kPpoMaxBlocks);
  hipStream_t s = (hipStream_t)stream;
  // with a control block the _ctl forms of the kernels, without one the plain forms: the code that ran before the block existed (amenv_train.hpp)
  if (ctl) hipLaunchKernelGGL(ppo_adv_partials_ctl, dim3(blocks), dim3(kPpoBlock), 0, s, (const amenv_ppo_ctl*)ctl, advantages, (int64_t)n, adv_part, (const int64_t*)nullptr);
  else hipLaunchKernelGGL(ppo_adv_partials, dim3(blocks), dim3(kPpoBlock), 0, s, advantages, (int64_t)n, adv_part, (const int64_t*)nullptr);
  (void)with_act_dim(act_dim, [&](auto a) {   // (a launch error is read below)
    if (old_values)   // the value-clip form, ctl or none; the launches around it are the _ctl or the plain ones
      hipLaunchKernelGGL(ppo_loss_grad_vclip<decltype(a)::value>, dim3(blocks), dim3(kPpoBlock), 0, s, (const amenv_ppo_ctl*)ctl, mean, value, log_std, actions, old_logp, advantages, returns,
                         (int64_t)n, clip_range, vf_coef, (int)normalize_advantage, (const double*)adv_part, blocks, d_mean, d_value, part, old_values, clip_range_vf);
    else if (ctl)
      hipLaunchKernelGGL(ppo_loss_grad_ctl<decltype(a)::value>, dim3(blocks), dim3(kPpoBlock), 0, s, (const amenv_ppo_ctl*)ctl, mean, value, log_std, actions, old_logp, advantages, returns,
                         (int64_t)n, clip_range, vf_coef, (int)normalize_advantage, (const double*)adv_part, blocks, d_mean, d_value, part);
    else
      hipLaunchKernelGGL(ppo_loss_grad<decltype(a)::value>, dim3(blocks), dim3(kPpoBlock), 0, s, mean, value, log_std, actions, old_logp, advantages, returns,
                         (int64_t)n, clip_range, vf_coef, (int)normalize_advantage, (const double*)adv_part, blocks, d_mean, d_value, part);
    return hipSuccess;
  });
  if (ctl) hipLaunchKernelGGL(ppo_finalize_ctl, dim3(1), dim3(64), 0, s, ctl, (const float*)part, blocks, (int)act_dim, (int64_t)n, log_std, ent_coef, d_log_std, stats4);
  else hipLaunchKernelGGL(ppo_finalize, dim3(1), dim3(64), 0, s, (const float*)part, blocks, (int)act_dim, (int64_t)n, log_std, ent_coef, d_log_std, stats4);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_ppo_loss_grad(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                        const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                        float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats4,
                        void* workspace, void* stream) {
  const int blocks = int(std::min<int64_t>(kPpoMaxBlocks, (n + kPpoBlock - 1) / kPpoBlock));
  return ppo_loss_grad_launch(mean, value, log_std, actions, old_logp, advantages, returns, n, act_dim, clip_range, ent_coef, vf_coef, normalize_advantage, d_mean,
                              d_value, d_log_std, stats4, workspace, nullptr, blocks, stream);
}

int amenv_ppo_loss_grad_ctl(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                            const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                            float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats4,
                            void* workspace, amenv_ppo_ctl* ctl, void* stream) {
  const int blocks = int(std::min<int64_t>(kPpoMaxBlocks, (n + kPpoBlock - 1) / kPpoBlock));
  return ppo_loss_grad_launch(mean, value, log_std, actions, old_logp, advantages, returns, n, act_dim, clip_range, ent_coef, vf_coef, normalize_advantage, d_mean,
                              d_value, d_log_std, stats4, workspace, ctl, blocks, stream);
}

int amenv_ppo_loss_grad_vclip(const float* mean, const float* value, const float* log_std, const float* actions, const float* old_logp,
                              const float* advantages, const float* returns, int64_t n, int32_t act_dim, float clip_range, float ent_coef,
                              float vf_coef, int32_t normalize_advantage, float* d_mean, float* d_value, float* d_log_std, float* stats4,
                              void* workspace, amenv_ppo_ctl* ctl, const float* old_values, float clip_range_vf, void* stream) {
  if (!old_values || !(clip_range_vf > 0.0f) || !std::isfinite(clip_range_vf)) return AMENV_ERR_INVALID;
  const int blocks = int(std::min<int64_t>(kPpoMaxBlocks, (n + kPpoBlock - 1) / kPpoBlock));
  return ppo_loss_grad_launch(mean, value, log_std, actions, old_logp, advantages, returns, n, act_dim, clip_range, ent_coef, vf_coef, normalize_advantage, d_mean,
                              d_value, d_log_std, stats4, workspace, ctl, blocks, stream, old_values, clip_range_vf);
}

size_t amenv_ppo_mlp_workspace_bytes(void) { return kMlpWsAdv + kMlpWsWt + kMlpWsPart; }

static int ppo_mlp_step_launch(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                               const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef, float vf_coef,
                               int32_t normalize_advantage, float* flat_grad, float* stats4, void* workspace, amenv_ppo_ctl* ctl, int adv_blocks, int blocks,
                               void* stream, const float* old_values = nullptr, float clip_range_vf = 0.0f) {
  if ((reinterpret_cast<uintptr_t>(ctl) & 3u) || !flat_params || !obs || !actions || !old_logp || !advantages || !returns || !flat_grad || !stats4 || !workspace || n <= 0 || !(clip_range >= 0.0f) ||
      (reinterpret_cast<uintptr_t>(workspace) & 15u) || !policy_shape_built(obs_dim, act_dim))
    return AMENV_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  double* adv_part = reinterpret_cast<double*>(ws);
  uint16_t* WS = reinterpret_cast<uint16_t*>(ws + kMlpWsAdv);
  float* part = reinterpret_cast<float*>(ws + kMlpWsAdv + kMlpWsWt);
  const dim3 pro_grid(adv_blocks + (2 * kMlpPackThreadsPerNet + kPpoBlock - 1) / kPpoBlock);
  if (ctl) hipLaunchKernelGGL(ppo_mlp_prologue_kernel_ctl, pro_grid, dim3(kPpoBlock), 0, s, (const amenv_ppo_ctl*)ctl, advantages, (int64_t)n, adv_part, index, adv_blocks, flat_params,
                              (int)obs_dim, (int)act_dim, WS);
  else hipLaunchKernelGGL(ppo_mlp_prologue_kernel, pro_grid, dim3(kPpoBlock), 0, s, advantages, (int64_t)n, adv_part, index, adv_blocks, flat_params, (int)obs_dim, (int)act_dim, WS);
  const hipError_t st = with_policy_shape(obs_dim, act_dim, [&](auto d, auto a) {
    constexpr int D_ = decltype(d)::value, A_ = decltype(a)::value;
    const u32x4* ws4 = reinterpret_cast<const u32x4*>(WS);
    if (old_values)   // the value-clip form, ctl or none
      return launch_mlp_step<true, D_, A_, true>(flat_params, ws4, obs, actions, old_logp, advantages, returns, index, n, clip_range, vf_coef, normalize_advantage, adv_part, adv_blocks,
                                                 part, blocks, ctl, s, old_values, clip_range_vf);
    return ctl ? launch_mlp_step<true, D_, A_>(flat_params, ws4, obs, actions, old_logp, advantages, returns, index, n, clip_range, vf_coef, normalize_advantage, adv_part, adv_blocks,
                                               part, blocks, ctl, s)
               : launch_mlp_step<false, D_, A_>(flat_params, ws4, obs, actions, old_logp, advantages, returns, index, n, clip_range, vf_coef, normalize_advantage, adv_part, adv_blocks,
                                                part, blocks, nullptr, s);
  });
  if (st != hipSuccess) return AMENV_ERR_HIP;
  const int trunk = kH1 * obs_dim + kH1 + kH2 * kH1 + kH2 + kH3 * kH2 + kH3;
  const int total = act_dim + 2 * trunk + act_dim * kH3 + act_dim + kH3 + 1;
  // plain form: the four scalars follow the gradient entries; _ctl form: one more workgroup that holds the scalars alone
  if (ctl)
    hipLaunchKernelGGL(mlp_grad_reduce_kernel_ctl, dim3((total + 63) / 64 + 1), dim3(64 * kRedGroups), 0, s, ctl, (const float*)part, blocks, (int)obs_dim, (int)act_dim, (int64_t)n,
                       flat_params, ent_coef, flat_grad, stats4);
  else
    hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((total + 4 + 63) / 64), dim3(64 * kRedGroups), 0, s, (const float*)part, blocks, (int)obs_dim, (int)act_dim, (int64_t)n, flat_params,
                       ent_coef, flat_grad, stats4);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_ppo_mlp_step(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                       const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef, float vf_coef,
                       int32_t normalize_advantage, float* flat_grad, float* stats4, void* workspace, void* stream) {
  const int adv_blocks = int(std::min<int64_t>(kPpoMaxBlocks, (n + kPpoBlock - 1) / kPpoBlock));
  const int64_t ntiles = (n + 31) / 32;
  const int blocks = int(std::min<int64_t>(128, (ntiles + 3) / 4));   // 128 x 2 nets x 4 wavefronts = one wavefront per SIMD
  return ppo_mlp_step_launch(flat_params, obs_dim, act_dim, obs, actions, old_logp, advantages, returns, index, n, clip_range, ent_coef, vf_coef, normalize_advantage,
                             flat_grad, stats4, workspace, nullptr, adv_blocks, blocks, stream);
}

int amenv_ppo_mlp_step_ctl(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                           const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef, float vf_coef,
                           int32_t normalize_advantage, float* flat_grad, float* stats4, void* workspace, amenv_ppo_ctl* ctl, void* stream) {
  const int adv_blocks = int(std::min<int64_t>(kPpoMaxBlocks, (n + kPpoBlock - 1) / kPpoBlock));
  const int64_t ntiles = (n + 31) / 32;
  const int blocks = int(std::min<int64_t>(128, (ntiles + 3) / 4));   // 128 x 2 nets x 4 wavefronts = one wavefront per SIMD
  return ppo_mlp_step_launch(flat_params, obs_dim, act_dim, obs, actions, old_logp, advantages, returns, index, n, clip_range, ent_coef, vf_coef, normalize_advantage,
                             flat_grad, stats4, workspace, ctl, adv_blocks, blocks, stream);
}

int amenv_ppo_mlp_step_vclip(const float* flat_params, int32_t obs_dim, int32_t act_dim, const float* obs, const float* actions, const float* old_logp,
                             const float* advantages, const float* returns, const int64_t* index, int64_t n, float clip_range, float ent_coef, float vf_coef,
                             int32_t normalize_advantage, float* flat_grad, float* stats4, void* workspace, amenv_ppo_ctl* ctl, const float* old_values,
                             float clip_range_vf, void* stream) {
  if (!old_values || !(clip_range_vf > 0.0f) || !std::isfinite(clip_range_vf)) return AMENV_ERR_INVALID;
  const int adv_blocks = int(std::min<int64_t>(kPpoMaxBlocks, (n + kPpoBlock - 1) / kPpoBlock));
  const int64_t ntiles = (n + 31) / 32;
  const int blocks = int(std::min<int64_t>(128, (ntiles + 3) / 4));   // 128 x 2 nets x 4 wavefronts = one wavefront per SIMD
  return ppo_mlp_step_launch(flat_params, obs_dim, act_dim, obs, actions, old_logp, advantages, returns, index, n, clip_range, ent_coef, vf_coef, normalize_advantage,
                             flat_grad, stats4, workspace, ctl, adv_blocks, blocks, stream, old_values, clip_range_vf);
}

static int ppo_adam_step_launch(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, const float* hyper6, float* grad_norm_out,
                                uint32_t* ticket, amenv_ppo_ctl* ctl, int blocks, void* stream) {
  if ((reinterpret_cast<uintptr_t>(ctl) & 3u) || !flat_params || !flat_grad || !exp_avg || !exp_avg_sq || !step || !hyper6 || !ticket || n <= 0 || !aligned16(flat_grad)) return AMENV_ERR_INVALID;
  if (ctl)
    hipLaunchKernelGGL(adam_clip_kernel_ctl, dim3(blocks), dim3(kAdamBlock), 0, (hipStream_t)stream, ctl, flat_params, (const float*)flat_grad, exp_avg, exp_avg_sq, step, (int64_t)n, hyper6,
                       grad_norm_out, ticket);
  else
    hipLaunchKernelGGL(adam_clip_kernel, dim3(blocks), dim3(kAdamBlock), 0, (hipStream_t)stream, flat_params, (const float*)flat_grad, exp_avg, exp_avg_sq, step, (int64_t)n, hyper6,
                       grad_norm_out, ticket);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

int amenv_ppo_adam_step(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, const float* hyper6, float* grad_norm_out,
                        uint32_t* ticket, void* stream) {
  const int blocks = int(std::min<int64_t>(kAdamMaxBlocks, (n + kAdamBlock - 1) / kAdamBlock));
  return ppo_adam_step_launch(flat_params, flat_grad, exp_avg, exp_avg_sq, step, n, hyper6, grad_norm_out, ticket, nullptr, blocks, stream);
}

int amenv_ppo_adam_step_ctl(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, const float* hyper6, float* grad_norm_out,
                            uint32_t* ticket, amenv_ppo_ctl* ctl, void* stream) {
  const int blocks = int(std::min<int64_t>(kAdamMaxBlocks, (n + kAdamBlock - 1) / kAdamBlock));
  return ppo_adam_step_launch(flat_params, flat_grad, exp_avg, exp_avg_sq, step, n, hyper6, grad_norm_out, ticket, ctl, blocks, stream);
}

// The KL-adaptive form: its own launch, the rule copied into it; geometry as amenv_ppo_adam_step's.
int amenv_ppo_adam_step_adapt(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* step, int64_t n, float* hyper6, float* grad_norm_out,
                              uint32_t* ticket, amenv_ppo_ctl* ctl, const amenv_ppo_lr_rule* rule, void* stream) {
  if (!ctl || (reinterpret_cast<uintptr_t>(ctl) & 3u) || !rule || rule->struct_size != sizeof(amenv_ppo_lr_rule)) return AMENV_ERR_INVALID;
  const amenv_ppo_lr_rule r = *rule;
  if (!std::isfinite(r.desired_kl) || !std::isfinite(r.band) || !std::isfinite(r.factor) || !std::isfinite(r.lr_min) || !std::isfinite(r.lr_max) ||
      !(r.desired_kl > 0.0f) || !(r.band >= 1.0f) || !(r.factor > 1.0f) || !(r.lr_min > 0.0f) || !(r.lr_min <= r.lr_max))
    return AMENV_ERR_INVALID;
  if (!flat_params || !flat_grad || !exp_avg || !exp_avg_sq || !step || !hyper6 || !ticket || n <= 0 || !aligned16(flat_grad)) return AMENV_ERR_INVALID;
  const int blocks = int(std::min<int64_t>(kAdamMaxBlocks, (n + kAdamBlock - 1) / kAdamBlock));
  hipLaunchKernelGGL(adam_clip_kernel_adapt, dim3(blocks), dim3(kAdamBlock), 0, (hipStream_t)stream, ctl, flat_params, (const float*)flat_grad, exp_avg, exp_avg_sq, step, (int64_t)n, hyper6,
                     grad_norm_out, ticket, r);
  return hipGetLastError() == hipSuccess ? AMENV_OK : AMENV_ERR_HIP;
}

}  // extern "C"
