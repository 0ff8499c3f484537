// amenv_capi_policy_norm.hip -- amenv_rollout_policy_norm, the closed-loop rollout with the observation normaliser inside: the one source that
// instantiates rollout_policy_kernel_rigid<.., NORM = true, ..>.  DESIGN 4x.
#include "amenv_rigid_policy_host.hpp"
#include "amenv_obsnorm.hpp"

extern "C" {

int amenv_rollout_policy_norm(amenv* e, amenv_obsnorm* h, int32_t update, float clip, double eps, int32_t n_steps, const float* flat_params, uint64_t seed,
                              uint32_t draw0, float* obs, float* actions, float* logp, float* values, float* rewards, uint8_t* dones, uint32_t* info_bits,
                              float* terminal_obs, void* stream) {
  if (!e || !h) return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: env and normaliser must be non-NULL");
  if (!rigid_pol_ok(e->cfg))
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: built for fp32 rigid vehicles with 4 or 6 rotors (arm vehicles: amenv_rollout_policy, normalise outside)");
  if (e->hist)
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: not built with the action history (amenv_set_action_history): normalise step by step, or turn the history off");
  if (h->dim != e->obs_dim) return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: the normaliser's dim differs from the env's obs_dim");
  if (h->device != e->device) return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: the normaliser lives on another device");
  if (n_steps <= 0 || !flat_params || !obs || !actions || !logp || !values || !rewards || !dones)
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: n_steps must be > 0 and flat_params / obs / actions / logp / values / rewards / dones non-NULL");
  if (!(clip > 0.0f) || !(eps >= 0.0)) return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: clip must be > 0 and eps >= 0");
  if (!aligned16(obs) || !aligned16(actions) || (terminal_obs && !aligned16(terminal_obs)))
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy_norm: obs / actions / terminal_obs must be 16-byte aligned");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  const PolicyIO io = policy_io(*e, flat_params, seed, draw0, obs, actions, logp, values, rewards, dones, info_bits, terminal_obs, s);
  AMENV_HIP(e, launch_rigid_policy<true>(*e, (int)n_steps, io, NormArg{h->buf, clip, eps, update}, s));
  const int d = h->dim;
  if (update)   // the launch left the sums of the raw rows 1..T in the batch slots: one merge of T x N rows (Chan's formula, associative)
    hipLaunchKernelGGL(obsnorm_merge_kernel, dim3(1), dim3(((d + 63) / 64) * 64), 0, s, h->buf, d, double(n_steps) * double(e->cfg.num_envs));
  AMENV_HIP(e, hipGetLastError());
  e->steps += uint64_t(e->cfg.num_envs) * uint64_t(n_steps);
  return AMENV_OK;
}

}  // extern "C"
