// amenv_rigid_policy_host.hpp -- launcher of rollout_policy_kernel_rigid, shared by the two sources that instantiate it: amenv_capi_policy.hip
// (NORM = false) and amenv_capi_policy_norm.hip (NORM = true).
#pragma once
#include "amenv_host.hpp"
#include "amenv_rigid_policy.hpp"

namespace {

// amenv_rigid_policy.hpp: workgroup shape by batch size: 16 envs per workgroup fill the CUs at small batches, 64 or 128 envs
// (one or two env wavefronts) cost fewer MLP wavefronts per env at large ones.  Measured on MI355X, v1_raw quadrotor with the normaliser, us per
// step (NE = 16 / 64 / 128): 4096 envs 5.4 / 7.4 / 11.0, 8192 9.4 / 7.3 / 10.9, 16384 17.5 / 7.9 / 11.3, 32768 33.3 / 14.3 / 12.0
// (profiles/r04/rigid_policy_crossover_*.json); the bounds sit at the interpolated crossovers.  -DAMENV_RIGID_WG16_MAX / -DAMENV_RIGID_WG64_MAX build the
// variants the crossover was measured with (tools/build_variant.py)
#ifndef AMENV_RIGID_WG16_MAX
#define AMENV_RIGID_WG16_MAX 6144
#endif
#ifndef AMENV_RIGID_WG64_MAX
#define AMENV_RIGID_WG64_MAX 24576
#endif
template <int NROT, int KW, int VAR, bool NORM, unsigned DYN>
hipError_t launch_rigid_policy_k(const amenv& e, int T, const PolicyIO& io, const NormArg& N, hipStream_t s) {
  const HotParams<float, NROT> HP = make_hot<float, NROT>(e);
  const ColdParams C = make_cold(e);
  const DynArg<float, NROT, DYN> R = make_dyn<float, NROT, DYN>(e);
  const int n = e.cfg.num_envs;
  if constexpr (NORM && (DYN & kDynDr) != 0) {
    if (e.fail.ctl != 0u) {   // the rotor failure inside the normaliser forms: instantiations of its own (amenv_rigid_policy.hpp, kDynFailForm)
      if (n <= AMENV_RIGID_WG16_MAX)
        hipLaunchKernelGGL((rollout_policy_kernel_rigid<NROT, KW, VAR, true, 16, (DYN | kDynFailForm)>), dim3(e.n_tiles * 4), dim3(320), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, C, N, R);
      else if (n <= AMENV_RIGID_WG64_MAX)
        hipLaunchKernelGGL((rollout_policy_kernel_rigid<NROT, KW, VAR, true, 64, (DYN | kDynFailForm)>), dim3(e.n_tiles), dim3(320), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, C, N, R);
      else
        hipLaunchKernelGGL((rollout_policy_kernel_rigid<NROT, KW, VAR, true, 128, (DYN | kDynFailForm)>), dim3(e.n_tiles / 2), dim3(384), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, C, N, R);
      return hipGetLastError();
    }
  }
  if (n <= AMENV_RIGID_WG16_MAX)
    hipLaunchKernelGGL((rollout_policy_kernel_rigid<NROT, KW, VAR, NORM, 16, DYN>), dim3(e.n_tiles * 4), dim3(320), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, C, N, R);
  else if (n <= AMENV_RIGID_WG64_MAX)
    hipLaunchKernelGGL((rollout_policy_kernel_rigid<NROT, KW, VAR, NORM, 64, DYN>), dim3(e.n_tiles), dim3(320), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, C, N, R);
  else   // (n_tiles is a multiple of 4: every 128-env workgroup covers two whole tiles)
    hipLaunchKernelGGL((rollout_policy_kernel_rigid<NROT, KW, VAR, NORM, 128, DYN>), dim3(e.n_tiles / 2), dim3(384), 0, s, e.blob, e.tile_bytes, n, T, io, e.stats, HP, C, N, R);
  return hipGetLastError();
}
template <bool NORM>
hipError_t launch_rigid_policy(const amenv& e, int T, const PolicyIO& io, const NormArg& N, hipStream_t s) {
  return with_rigid_form<float>(e, [&](auto nrot, auto dyn) {
    if constexpr (decltype(nrot)::value == 4 || decltype(nrot)::value == 6)   // (rigid_pol_ok)
      return with_task(e, [&](auto kw, auto var) {
        return launch_rigid_policy_k<decltype(nrot)::value, decltype(kw)::value, decltype(var)::value, NORM, decltype(dyn)::value>(e, T, io, N, s);
      });
    else return hipErrorInvalidValue;
  });
}

}  // namespace
