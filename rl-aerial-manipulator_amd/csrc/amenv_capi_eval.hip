// amenv_capi_eval.hip -- amenv_evaluate_policy, the one-launch evaluation: the one source that instantiates evaluate_policy_kernel_*.  DESIGN 4x.
#include "amenv_host.hpp"
#include "amenv_eval_policy.hpp"

namespace {

// amenv_evaluate_policy (amenv_eval_policy.hpp): one workgroup shape at every batch size -- 16 envs for the rigid vehicles, 64 for the arm
template <bool NORM>
hipError_t launch_rigid_eval(const amenv& e, int max_steps, const PolicyIO& io, const NormArg& N, const EvalArg& E, hipStream_t s) {
  return with_rigid_form<float>(e, [&](auto nrot, auto dyn) {
    if constexpr (decltype(nrot)::value == 4 || decltype(nrot)::value == 6)   // (rigid_pol_ok)
      return with_task(e, [&](auto kw, auto var) {
        constexpr int NROT = decltype(nrot)::value;
        constexpr unsigned DYN = decltype(dyn)::value;
        hipLaunchKernelGGL((evaluate_policy_kernel_rigid<NROT, decltype(kw)::value, decltype(var)::value, NORM, DYN>), dim3(e.n_tiles * 4), dim3(320), 0, s, e.blob, e.tile_bytes,
                           e.cfg.num_envs, max_steps, io, make_hot<float, NROT>(e), make_cold(e), N, make_dyn<float, NROT, DYN>(e), E);
        return hipGetLastError();
      });
    else return hipErrorInvalidValue;
  });
}
template <int KW, int PNJ>
hipError_t launch_lane_eval_k(const amenv& e, int max_steps, const PolicyIO& io, const EvalArg& E, hipStream_t s) {
  ArmArg<float, 3> AA;
  AA.p = make_arm<float>(e);
  hipLaunchKernelGGL((evaluate_policy_kernel_lane<KW, PNJ>), dim3(e.n_tiles), dim3(320), 0, s, e.blob, e.tile_bytes, e.cfg.num_envs, max_steps, io, make_hot<float, 6>(e), make_cold(e), AA, E);
  return hipGetLastError();
}
template <int KW>
hipError_t launch_lane_eval_kw(const amenv& e, int max_steps, const PolicyIO& io, const EvalArg& E, hipStream_t s) {
  if (e.pub_nj == 1) return launch_lane_eval_k<KW, 1>(e, max_steps, io, E, s);
  if (e.pub_nj == 2) return launch_lane_eval_k<KW, 2>(e, max_steps, io, E, s);
  return launch_lane_eval_k<KW, 3>(e, max_steps, io, E, s);
}
hipError_t launch_lane_eval(const amenv& e, int max_steps, const PolicyIO& io, const EvalArg& E, hipStream_t s) {
  return e.cfg.task.num_waypoints == 1 ? launch_lane_eval_kw<1>(e, max_steps, io, E, s) : launch_lane_eval_kw<AMENV_MAX_WAYPOINTS>(e, max_steps, io, E, s);
}

}  // namespace

extern "C" {

int amenv_evaluate_policy(amenv* e, amenv_obsnorm* h, float clip, double eps, const float* flat_params, int32_t deterministic, uint64_t seed, uint32_t draw0,
                          int32_t episodes_per_env, int32_t max_steps, double* returns, int32_t* counts, int32_t* steps_run, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!flat_params || !returns || !counts || !steps_run) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: flat_params / returns / counts / steps_run must be non-NULL");
  if (episodes_per_env <= 0 || max_steps <= 0) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: episodes_per_env and max_steps must be > 0");
  if (e->cfg.dtype != AMENV_F32) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: built for fp32 handles (an fp64 handle evaluates step by step)");
  if (!(e->cfg.flags & AMENV_FLAG_AUTO_RESET))
    return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: needs AMENV_FLAG_AUTO_RESET (an env whose episode ended would never start the next one)");
  const bool rigid = rigid_pol_ok(e->cfg), arm = arm_pol_ok(e->cfg);
  if (!rigid && !arm)
    return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: built for rigid vehicles with 4 or 6 rotors (every task) and the 6-rotor vehicle with a 1..3-link arm (v2 task)");
  if (h) {
    if (!rigid) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: the normaliser form is built for rigid vehicles (arm vehicles: norm = NULL)");
    if (e->hist) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: the normaliser form is not built with the action history (amenv_set_action_history)");
    if (h->dim != e->obs_dim) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: the normaliser's dim differs from the env's obs_dim");
    if (h->device != e->device) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: the normaliser lives on another device");
    if (!(clip > 0.0f) || !(eps >= 0.0)) return fail(e, AMENV_ERR_INVALID, "amenv_evaluate_policy: clip must be > 0 and eps >= 0");
  }
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  AMENV_HIP(e, hipMemsetAsync(steps_run, 0, sizeof(int32_t), s));
  const PolicyIO io = policy_io(*e, flat_params, seed, draw0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s);
  const EvalArg E{deterministic, episodes_per_env, returns, counts, steps_run};
  if (!rigid) AMENV_HIP(e, launch_lane_eval(*e, (int)max_steps, io, E, s));
  else if (h) AMENV_HIP(e, launch_rigid_eval<true>(*e, (int)max_steps, io, NormArg{h->buf, clip, eps, 0}, E, s));
  else AMENV_HIP(e, launch_rigid_eval<false>(*e, (int)max_steps, io, NormArg{nullptr, 0.0f, 0.0, 0}, E, s));
  return AMENV_OK;   // (the step counter behind amenv_stats is host-side and stays: the steps executed are known on the device only)
}

}  // extern "C"
