// amenv_capi_step.hip -- amenv_step / amenv_step_timed (and the AMENV_STAMPS debug entry points): the one source that instantiates the
// step kernels of every family (step_kernel, _pw, _team, _armk, _arm2w, _quad).  DESIGN 4x.
#include "amenv_host.hpp"

namespace {

// amenv_step (timed: amenv_step_timed) with one instantiation of the kernel templates (amenv_rollout: amenv_capi_rollout.hip); the
// if constexpr guards keep every kernel out of the code object that no config pairs with this instantiation
template <typename T, int NROT, int KW, int VAR, int NJ = 0, unsigned DYN = 0>
hipError_t launch_step(const amenv& e, const StepIO& io, hipStream_t s, bool timed) {
  ArmArg<T, NJ> AA;
  if constexpr (NJ > 0) AA.p = make_arm<T>(e); else AA.unused = 0;
  const HotParams<T, NROT> P = make_hot<T, NROT>(e);
  const ColdParams C = make_cold(e);
  const StepTail tl{io.terminal_obs, io.ep_return, io.ep_len, io.stats};
  const uint32_t tb = e.tile_bytes;
  const int32_t n = e.cfg.num_envs;
  switch (e.family) {
    case StepFamily::Team:   // 16 lanes per env; 16 envs per workgroup (four main waves + one episode-end helper wave) while each workgroup has a CU to itself, else 4 (one + one)
      if constexpr (NJ == 3 && DYN == 0) {   // (the kernel reads its parameters from the device block behind the table: amenv_create wrote them there)
        const TeamParamsT<T> TP = make_team<T>(e);
        if (team_wide(e))
          return launch(e, timed, step_kernel_team<T, NROT, 4>, dim3(e.n_tiles * 4), dim3(320), 0, s, e.blob, n, int32_t(e.n_tiles * 4),
                        reinterpret_cast<const float*>(io.actions), TP.consts, io.obs, static_cast<T*>(io.reward), io.done, io.info, tl, C);
        return launch(e, timed, step_kernel_team<T, NROT, 1>, dim3(e.n_tiles * 16), dim3(128), 0, s, e.blob, n, int32_t(e.n_tiles * 16),
                      reinterpret_cast<const float*>(io.actions), TP.consts, io.obs, static_cast<T*>(io.reward), io.done, io.info, tl, C);
      }
      break;
    case StepFamily::Staged:   // one tile per 320-thread workgroup: four stage waves + main wave
      if constexpr (NJ == 3 && DYN == 0) {
        if constexpr (sizeof(T) == 8) {   // the fp64 logic-gate build exchanges its aggregates in fp64: > 64 KB of dynamic LDS needs the attribute
          hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&step_kernel_armk<T, NROT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
          if (ea != hipSuccess) return ea;
        }
        const size_t lds = size_t(64 * ObsDim<VAR, NJ>::value + 12 * 64) * sizeof(float) + size_t((4 * kAggSlots + 6) * 64) * sizeof(T);   // obs rows | reset words | aggregates, joints (T)
        return launch(e, timed, step_kernel_armk<T, NROT>, dim3(e.n_tiles), dim3(320), lds, s, e.blob, tb, n, io.actions, io.obs, io.reward, io.done, io.info, tl, P, C, AA);
      }
      break;
    case StepFamily::TwoWave:   // one tile per 128-thread workgroup: main + helper wave
      if constexpr (NJ == 3 && sizeof(T) == 4 && DYN == 0) {
        const size_t lds = size_t(64 * ObsDim<VAR, NJ>::value + (kArmXchgSlots + 12) * 64) * sizeof(float);   // obs rows | RK4 exchange | reset words
        return launch(e, timed, step_kernel_arm2w<T, NROT>, dim3(e.n_tiles), dim3(128), lds, s, e.blob, tb, n, io.actions, io.obs, io.reward, io.done, io.info, tl, P, C, AA);
      }
      break;
    case StepFamily::Quad:   // 4 lanes per env, 16 envs per workgroup: main wave + episode-end helper wave
      if constexpr (NJ == 0 && sizeof(T) == 4 && KW == 1 && VAR == VAR_V2 && (NROT == 4 || NROT == 6) && DYN == 0)
        return launch(e, timed, step_kernel_quad<NROT>, dim3(e.n_tiles * 4), dim3(128), 0, s, e.blob, tb, n, io.actions, io.obs, static_cast<float*>(io.reward), io.done,
                      io.info, tl, C, make_quad(e));
      break;
    case StepFamily::LaneHelper:   // one tile per workgroup: main wave + reset-RNG wave (+ observation and Monitor waves for the single-waypoint v2 task)
      if constexpr (NJ == 0) {
        const size_t lds = size_t(64 * (ObsDim<VAR, 0>::value + ((DYN & kDynDelay) ? 8 : 0)) + 12 * 64) * sizeof(float);   // (the DELAY forms stage rows of up to two more action rows)
        if constexpr (sizeof(T) == 8 && (DYN & kDynDr) != 0) {   // fp64 with the rotor failure set: the forms that carry its code (kDynFailForm)
          if (e.fail.ctl != 0u)
            return launch(e, timed, step_kernel_pw<T, NROT, KW, VAR, (DYN | kDynFailForm)>, dim3(e.n_tiles), dim3((KW == 1 && VAR == VAR_V2) ? 256 : 128), lds, s, e.blob, tb, n,
                          io.actions, io.obs, io.reward, io.done, io.info, tl, P, C, make_dyn<T, NROT, DYN>(e));
        }
        return launch(e, timed, step_kernel_pw<T, NROT, KW, VAR, DYN>, dim3(e.n_tiles), dim3((KW == 1 && VAR == VAR_V2) ? 256 : 128), lds, s, e.blob, tb, n, io.actions,
                      io.obs, io.reward, io.done, io.info, tl, P, C, make_dyn<T, NROT, DYN>(e));
      }
      break;
    case StepFamily::Lane: {
      const int bs = e.block;
      if constexpr (sizeof(T) == 8 && (DYN & kDynDr) != 0) {   // (as above)
        if (e.fail.ctl != 0u)
          return launch(e, timed, step_kernel<T, NROT, KW, VAR, NJ, (DYN | kDynFailForm)>, dim3((e.n_tiles * 64 + bs - 1) / bs), dim3(bs), size_t(bs) * ObsDim<VAR, NJ>::value * sizeof(float), s,
                        e.blob, tb, n, io.actions, io.obs, io.reward, io.done, io.info, tl, P, C, AA, make_dyn<T, NROT, DYN>(e));
      }
      return launch(e, timed, step_kernel<T, NROT, KW, VAR, NJ, DYN>, dim3((e.n_tiles * 64 + bs - 1) / bs), dim3(bs), size_t(bs) * (ObsDim<VAR, NJ>::value + ((DYN & kDynDelay) ? 4 * e.hist : 0)) * sizeof(float), s,
                    e.blob, tb, n, io.actions, io.obs, io.reward, io.done, io.info, tl, P, C, AA, make_dyn<T, NROT, DYN>(e));
    }
  }
  return hipErrorInvalidValue;   // a family this instantiation has no kernel for: select_step_family and dispatch_step never pair them
}

// The launchers below pick the handle's arithmetic type themselves: behind each template a plain overload that the entry points call
template <typename T>
hipError_t dispatch_step(const amenv& e, const StepIO& io, hipStream_t s, bool timed) {
  if (e.cfg.vehicle.n_joints == 3) {
    if (e.cfg.task.num_waypoints == 1) return launch_step<T, 6, 1, VAR_V2, 3>(e, io, s, timed);   // BASELINE config 3
    return launch_step<T, 6, AMENV_MAX_WAYPOINTS, VAR_V2, 3>(e, io, s, timed);                    // arm + 2..4 waypoints: the lane kernel
  }
  return with_rigid_form<T>(e, [&](auto nrot, auto dyn) {
    return with_task(e, [&](auto kw, auto var) {
      return launch_step<T, decltype(nrot)::value, decltype(kw)::value, decltype(var)::value, 0, decltype(dyn)::value>(e, io, s, timed);
    });
  });
}
hipError_t dispatch_step(const amenv& e, const StepIO& io, hipStream_t s, bool timed) { return e.cfg.dtype == AMENV_F64 ? dispatch_step<double>(e, io, s, timed) : dispatch_step<float>(e, io, s, timed); }

}  // namespace

extern "C" {

namespace {
// amenv_step and amenv_step_timed after their NULL checks (who: the entry point, for the messages)
int step_launch(amenv* e, const char* who, const float* actions, float* obs, void* reward, uint8_t* done, uint32_t* info_bits, float* terminal_obs,
                float* ep_return, int32_t* ep_len, hipStream_t s, bool timed) {
  if (!aligned16(actions) || !aligned16(obs) || (terminal_obs && !aligned16(terminal_obs)))
    return fail(e, AMENV_ERR_INVALID, std::string(who) + ": actions/obs/terminal_obs must be 16-byte aligned");
  DeviceGuard g(e->device);
  StepIO io{reinterpret_cast<const float4*>(actions), obs, reward, done, info_bits, terminal_obs, ep_return, ep_len, e->stats};
  if (e->io_act) { AMENV_HIP(e, pad_actions(*e, actions, s)); io.actions = reinterpret_cast<const float4*>(e->io_act); io.obs = e->io_obs; io.terminal_obs = terminal_obs ? e->io_term : nullptr; }
  AMENV_HIP(e, dispatch_step(*e, io, s, timed));
  if (e->io_act) { AMENV_HIP(e, cut_obs(*e, e->io_obs, nullptr, obs, s)); if (terminal_obs) AMENV_HIP(e, cut_obs(*e, e->io_term, done, terminal_obs, s)); }
  e->steps += uint64_t(e->cfg.num_envs);
  return AMENV_OK;
}
}  // namespace

int amenv_step(amenv* e, const float* actions, float* obs, void* reward, uint8_t* done, uint32_t* info_bits, float* terminal_obs,
               float* ep_return, int32_t* ep_len, void* stream) {
  if (!e) return AMENV_ERR_INVALID;
  if (!actions || !obs || !reward || !done || !info_bits) return fail(e, AMENV_ERR_INVALID, "amenv_step: actions/obs/reward/done/info_bits must be non-NULL");
  return step_launch(e, "amenv_step", actions, obs, reward, done, info_bits, terminal_obs, ep_return, ep_len, (hipStream_t)stream, false);
}

int amenv_step_timed(amenv* e, const float* actions, float* obs, void* reward, uint8_t* done, uint32_t* info_bits,
                     float* terminal_obs, float* ep_return, int32_t* ep_len, void* stream, float* kernel_us) {
  if (!e) return AMENV_ERR_INVALID;
  if (!actions || !obs || !reward || !done || !info_bits || !kernel_us) return fail(e, AMENV_ERR_INVALID, "amenv_step_timed: NULL argument");
  DeviceGuard g(e->device);
  if (!e->ev_start) { AMENV_HIP(e, hipEventCreate(&e->ev_start)); AMENV_HIP(e, hipEventCreate(&e->ev_stop)); }
  const int rc = step_launch(e, "amenv_step_timed", actions, obs, reward, done, info_bits, terminal_obs, ep_return, ep_len, (hipStream_t)stream, true);
  if (rc != AMENV_OK) return rc;
  AMENV_HIP(e, hipEventSynchronize(e->ev_stop));
  float ms = 0.f;
  AMENV_HIP(e, hipEventElapsedTime(&ms, e->ev_start, e->ev_stop));
  *kernel_us = ms * 1000.0f;
  return AMENV_OK;
}

#ifdef AMENV_STAMPS
// diagnostic build only: an empty kernel with the step kernel's grid, to measure the dependent-launch floor
__global__ void noop_kernel(void* blob, uint32_t tile_bytes, int32_t n, unsigned long long* sink) {
  if (n < 0) sink[0] = tile_bytes;
}
__global__ void touch_kernel(void* blob, uint32_t tile_bytes, int32_t n, unsigned long long* sink) {
  // one 16-B load + one 16-B store per lane: the minimal memory round trip
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int4* p = reinterpret_cast<int4*>(static_cast<char*>(blob) + size_t(i >> 6) * tile_bytes) + (threadIdx.x & 63);
  int4 v = *p; v.w ^= 0; *p = v;
}
int amenv_debug_noop(amenv* e, int which, int block, void* stream) {
  DeviceGuard g(e->device);
  const int bs = block > 0 ? block : e->block, n_pad = e->n_tiles * 64;
  if (which >= 2) hipLaunchKernelGGL(noop_kernel, dim3(which), dim3(bs), 0, (hipStream_t)stream, e->blob, e->tile_bytes, e->cfg.num_envs, e->stats);   // explicit grid
  else if (which == 0) hipLaunchKernelGGL(noop_kernel, dim3((n_pad + bs - 1) / bs), dim3(bs), 0, (hipStream_t)stream, e->blob, e->tile_bytes, e->cfg.num_envs, e->stats);
  else hipLaunchKernelGGL(touch_kernel, dim3((n_pad + bs - 1) / bs), dim3(bs), 0, (hipStream_t)stream, e->blob, e->tile_bytes, e->cfg.num_envs, e->stats);
  AMENV_HIP(e, hipGetLastError());
  return AMENV_OK;
}

// diagnostic build only: copy the per-wave s_memtime stamps of the last step launch to host (synchronises)
int amenv_debug_stamps(amenv* e, unsigned long long* host_out /*[64][8]*/) {
  DeviceGuard g(e->device);
  AMENV_HIP(e, hipDeviceSynchronize());
  AMENV_HIP(e, hipMemcpy(host_out, e->stats + kStampBase, sizeof(unsigned long long) * kStampWaves * kStampSlots, hipMemcpyDeviceToHost));
  return AMENV_OK;
}
#endif

}  // extern "C"
