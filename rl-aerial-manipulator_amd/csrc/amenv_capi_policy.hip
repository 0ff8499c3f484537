// amenv_capi_policy.hip -- amenv_rollout_policy, the one-launch closed-loop rollout: the one source that instantiates
// rollout_policy_kernel_rigid<.., NORM = false, ..>, rollout_policy_kernel_quad, _team and _lane.  DESIGN 4x.
#include "amenv_rigid_policy_host.hpp"
#include "amenv_team_policy.hpp"
#include "amenv_quad_policy.hpp"
#include "amenv_lane_policy.hpp"

namespace {

// amenv_rollout_policy, arm vehicles outside the team kernel's range: one lane per env (amenv_lane_policy.hpp; 64 envs per workgroup up to
// 16384 envs, 128 above: one workgroup per CU either way).  PNJ: the caller's joints (a 1- / 2-link arm publishes its own row widths)
template <int KW, int PNJ>
hipError_t launch_lane_policy_k(const amenv& e, int T, const PolicyIO& io, hipStream_t s) {
  ArmArg<float, 3> AA;
  AA.p = make_arm<float>(e);
  const HotParams<float, 6> HP = make_hot<float, 6>(e);
  const int n = e.cfg.num_envs;
  if (n <= 16384)
    hipLaunchKernelGGL((rollout_policy_kernel_lane<6, 1, KW, PNJ>), dim3(e.n_tiles), dim3(320), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, make_cold(e), AA, e.io_term);
  else
    hipLaunchKernelGGL((rollout_policy_kernel_lane<6, 2, KW, PNJ>), dim3((e.n_tiles + 1) / 2), dim3(384), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, make_cold(e), AA,
                       e.io_term);
  return hipGetLastError();
}
template <int KW>
hipError_t launch_lane_policy_kw(const amenv& e, int T, const PolicyIO& io, hipStream_t s) {
  if (e.pub_nj == 1) return launch_lane_policy_k<KW, 1>(e, T, io, s);
  if (e.pub_nj == 2) return launch_lane_policy_k<KW, 2>(e, T, io, s);
  return launch_lane_policy_k<KW, 3>(e, T, io, s);
}
hipError_t launch_lane_policy(const amenv& e, int T, const PolicyIO& io, hipStream_t s) {
  return e.cfg.task.num_waypoints == 1 ? launch_lane_policy_kw<1>(e, T, io, s) : launch_lane_policy_kw<AMENV_MAX_WAYPOINTS>(e, T, io, s);
}

}  // namespace

extern "C" {

int amenv_rollout_policy(amenv* e, int32_t n_steps, const float* flat_params, uint64_t seed, uint32_t draw0, float* obs, float* actions, float* logp,
                         float* values, float* rewards, uint8_t* dones, uint32_t* info_bits, float* terminal_obs, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  // with dynamics randomisation a quad_ok config runs the one-lane-per-env form: the lane-quad kernels are not built with it
  const bool quad = !e->dr && !e->lag && !e->noise && !e->delay_path() && !e->rate.on && !e->fail.ctl && quad_ok(e->cfg), rigid = !quad && rigid_pol_ok(e->cfg);
  if (!quad && !rigid && !arm_pol_ok(e->cfg))
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy: built for fp32 vehicles: rigid with 4 or 6 rotors (every task), or the 6-rotor vehicle with a "
                "1..3-link arm (v2 task, 1..4 waypoints, any joint axes)");
  if (n_steps <= 0 || !flat_params || !obs || !actions || !logp || !values || !rewards || !dones)
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy: n_steps must be > 0 and flat_params / obs / actions / logp / values / rewards / dones non-NULL");
  if (rigid && (!aligned16(obs) || !aligned16(actions) || (terminal_obs && !aligned16(terminal_obs))))
    return fail(e, AMENV_ERR_INVALID, "amenv_rollout_policy: obs / actions / terminal_obs must be 16-byte aligned");
  DeviceGuard g(e->device);
  hipStream_t s = (hipStream_t)stream;
  const PolicyIO io = policy_io(*e, flat_params, seed, draw0, obs, actions, logp, values, rewards, dones, info_bits, terminal_obs, s);
  const int n = e->cfg.num_envs;
  if (quad) {   // rigid vehicle, single-waypoint v2 task, default workgroup size: 16 envs per workgroup, the lane-quad step inside (amenv_quad_policy.hpp)
    const QuadParams QP = make_quad(*e);
    const dim3 gq(e->n_tiles * 4), bq(256);
    with_rotors46(e->cfg.vehicle.n_rotors, [&](auto nrot) {
      hipLaunchKernelGGL((rollout_policy_kernel_quad<decltype(nrot)::value>), gq, bq, 0, s, e->blob, e->tile_bytes, n, (int)n_steps, io, e->stats, make_cold(*e), QP);
    });
  } else if (rigid) {   // every other rigid config (v1 tasks, 2..4 waypoints, a set workgroup size): one lane per env (amenv_rigid_policy.hpp)
    AMENV_HIP(e, launch_rigid_policy<false>(*e, (int)n_steps, io, NormArg{nullptr, 0.0f, 0.0, 0}, s));
  } else if (e->family == StepFamily::Team && !e->io_act) {   // the caller's vehicle is the 3-joint z,x,x arm on one waypoint
    // The env part follows the step kernel's choice: 16 lanes per env where amenv_step runs the lane-team kernel (small batches).  One 16-env
    // workgroup per CU up to 4096 envs (5.15 vs 5.22 us per step there); above that the variant compiled for two wavefronts per SIMD pays
    // (measured on MI355X at 8192 envs: 7.9 vs 10.1 us per step)
    const TeamParams TP = make_team<float>(*e);
    if (n <= 4096) hipLaunchKernelGGL((rollout_policy_kernel_team<6, 1>), dim3(e->n_tiles * 4), dim3(256), 0, s, e->blob, e->tile_bytes, n, (int)n_steps, io, e->stats, make_cold(*e), TP);
    else hipLaunchKernelGGL((rollout_policy_kernel_team<6, 2>), dim3(e->n_tiles * 4), dim3(256), 0, s, e->blob, e->tile_bytes, n, (int)n_steps, io, e->stats, make_cold(*e), TP);
  } else {   // every other fp32 arm config: one lane per env
    AMENV_HIP(e, launch_lane_policy(*e, (int)n_steps, io, s));
  }
  AMENV_HIP(e, hipGetLastError());
  e->steps += uint64_t(e->cfg.num_envs) * uint64_t(n_steps);
  return AMENV_OK;
}

}  // extern "C"
