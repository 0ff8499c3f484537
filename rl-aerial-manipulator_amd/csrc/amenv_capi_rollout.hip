// amenv_capi_rollout.hip -- amenv_rollout, the open-loop rollout: the one source that instantiates rollout_kernel, rollout_kernel_team and
// rollout_kernel_quad.  DESIGN 4x.
#include "amenv_host.hpp"

namespace {

// amenv_rollout, T_steps steps in one launch: the team and quad families have rollout kernels of their own, every other family's rollout
// runs the lane kernel
template <typename T, int NROT, int KW, int VAR, int NJ, unsigned DYN>
hipError_t launch_rollout(const amenv& e, const StepIO& io, int T_steps, hipStream_t s) {
  const StepTail tl{io.terminal_obs, io.ep_return, io.ep_len, io.stats};
  const ColdParams C = make_cold(e);
  const uint32_t tb = e.tile_bytes;
  const int32_t n = e.cfg.num_envs;
  switch (e.family) {
    case StepFamily::Team:   // one wave per 4 envs; the fp64 build is a logic gate of amenv_step only (amenv_rollout refuses it)
      if constexpr (NJ == 3 && sizeof(T) == 4 && DYN == 0)
        return launch(e, false, rollout_kernel_team<NROT>, dim3(e.n_tiles * 16), dim3(64), 0, s, e.blob, tb, n, reinterpret_cast<const float*>(io.actions), io.obs,
                      static_cast<float*>(io.reward), io.done, io.info, T_steps, tl, C, make_team<T>(e));
      return hipErrorInvalidValue;
    case StepFamily::Quad:   // one wave per 16 envs
      if constexpr (NJ == 0 && sizeof(T) == 4 && KW == 1 && VAR == VAR_V2 && (NROT == 4 || NROT == 6) && DYN == 0)
        return launch(e, false, rollout_kernel_quad<NROT>, dim3(e.n_tiles * 4), dim3(64), 0, s, e.blob, tb, n, io.actions, io.obs, static_cast<float*>(io.reward), io.done,
                      io.info, T_steps, tl, C, make_quad(e));
      return hipErrorInvalidValue;
    case StepFamily::Lane: case StepFamily::LaneHelper: case StepFamily::Staged: case StepFamily::TwoWave:
      break;
  }
  ArmArg<T, NJ> AA;
  if constexpr (NJ > 0) AA.p = make_arm<T>(e); else AA.unused = 0;
  const int bs = e.block;
  return launch(e, false, rollout_kernel<T, NROT, KW, VAR, NJ, DYN>, dim3((e.n_tiles * 64 + bs - 1) / bs), dim3(bs), size_t(bs) * (ObsDim<VAR, NJ>::value + ((DYN & kDynDelay) ? 4 * e.hist : 0)) * sizeof(float), s,
                e.blob, tb, n, io.actions, io.obs, io.reward, io.done, io.info, T_steps, tl, make_hot<T, NROT>(e), C, AA, make_dyn<T, NROT, DYN>(e));
}

// the handle's instantiation of launch_rollout: dispatch_step's walk (amenv_capi_step.hip) over the same visitors
template <typename T>
hipError_t dispatch_rollout(const amenv& e, const StepIO& io, int T_steps, hipStream_t s) {
  if (e.cfg.vehicle.n_joints == 3) {
    if (e.cfg.task.num_waypoints == 1) return launch_rollout<T, 6, 1, VAR_V2, 3, 0>(e, io, T_steps, s);   // BASELINE config 3
    return launch_rollout<T, 6, AMENV_MAX_WAYPOINTS, VAR_V2, 3, 0>(e, io, T_steps, s);                    // arm + 2..4 waypoints: the lane kernel
  }
  return with_rigid_form<T>(e, [&](auto nrot, auto dyn) {
    return with_task(e, [&](auto kw, auto var) {
      return launch_rollout<T, decltype(nrot)::value, decltype(kw)::value, decltype(var)::value, 0, decltype(dyn)::value>(e, io, T_steps, s);
    });
  });
}
hipError_t dispatch_rollout(const amenv& e, const StepIO& io, int T_steps, hipStream_t s) { return e.cfg.dtype == AMENV_F64 ? dispatch_rollout<double>(e, io, T_steps, s) : dispatch_rollout<float>(e, io, T_steps, s); }

}  // namespace

extern "C" {

int amenv_rollout(amenv* e, int32_t n_steps, const float* actions, float* obs, void* reward, uint8_t* done, uint32_t* info_bits,
                  void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (n_steps <= 0 || !actions) return fail(e, AMENV_ERR_INVALID, "amenv_rollout: n_steps must be > 0 and actions non-NULL");
  if (!aligned16(actions) || (obs && !aligned16(obs))) return fail(e, AMENV_ERR_INVALID, "amenv_rollout: actions/obs must be 16-byte aligned");
  if (e->family == StepFamily::Team && e->cfg.dtype == AMENV_F64) return fail(e, AMENV_ERR_INVALID, "amenv_rollout: the fp64 lane-team build is a logic gate of amenv_step only");
  if (e->io_act) return fail(e, AMENV_ERR_INVALID, "amenv_rollout: arms with 1 or 2 joints are served through amenv_step (the adapters at the C ABI are per step)");
  DeviceGuard g(e->device);
  StepIO io{reinterpret_cast<const float4*>(actions), obs, reward, done, info_bits, nullptr, nullptr, nullptr, e->stats};
  hipError_t st = dispatch_rollout(*e, io, n_steps, (hipStream_t)stream);
  AMENV_HIP(e, st);
  e->steps += uint64_t(e->cfg.num_envs) * uint64_t(n_steps);
  return AMENV_OK;
}

}  // extern "C"
