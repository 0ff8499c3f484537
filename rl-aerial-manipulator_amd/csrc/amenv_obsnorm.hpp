// amenv_obsnorm.hpp -- GPU running observation normaliser, the on-device equivalent of
// `VecNormalize(env, norm_obs=True, norm_reward=False)` (v1/rl_train_vecN.py:10-11, v1/rl_checkpoint_train_vecN.py:19-26).
// Third-party semantics (stable-baselines3 2.6.0, common/running_mean_std.py + vec_normalize.py; not vendored by the
// reference, its vec_normalize.pkl is a pickle and is never loaded): running mean / population variance / count
// (initial 0 / 1 / 1e-4) merged with each batch by the parallel-moments formula, then
// obs_n = clip((obs - mean) / sqrt(var + 1e-8), -10, 10).  Parity unpinned; checked against a numpy restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amenv_dev {

// buffer layout (doubles): [0,d) mean | [d,2d) var | [2d] count | [2d+1, 3d+1) batch sum | [3d+1, 4d+1) batch sum of squares
__host__ __device__ inline int obsnorm_words(int d) { return 4 * d + 1; }

// The kernels (bodies: amenv_obsnorm_kernels.hpp, which ONE source includes -- amenv_capi.hip; amenv_capi_policy_norm.hip launches the merge through
// this declaration)
__global__ __launch_bounds__(256) void obsnorm_sum_kernel(const float* __restrict__ obs, long long n_elems, int d, long long stride,
                                                          double* __restrict__ buf);
__global__ void obsnorm_merge_kernel(double* __restrict__ buf, int d, double batch_count);
__global__ __launch_bounds__(256) void obsnorm_apply_kernel(const float* __restrict__ in, float* __restrict__ out, long long n_elems, int d,
                                                            const double* __restrict__ buf, float clip, double eps);

}  // namespace amenv_dev
