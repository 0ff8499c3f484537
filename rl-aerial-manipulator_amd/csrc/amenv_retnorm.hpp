// amenv_retnorm.hpp -- GPU return-based reward normaliser, the on-device equivalent of the reward half of
// `VecNormalize(env, norm_reward=True)`.  Third-party semantics (stable-baselines3 2.6.0, common/vec_normalize.py +
// running_mean_std.py; SB3's default, the reference itself trains with norm_reward=False, v1/rl_train_vecN.py:11), restated:
//   state: returns[N] (fp64, zero after reset()), ret_rms = scalar running mean / population variance / count (0 / 1 / 1e-4)
//   per env step t, training:  1. returns = returns * gamma + r_t
//                              2. ret_rms.update(returns): merge the batch (mean, np.var, N) by the parallel-moments formula
//                              3. out_t = clip(r_t / sqrt(ret_rms.var + eps), -clip, clip)      (the variance AFTER step 2)
//                              4. returns[done_t] = 0
//   not training: 1, 2 and 4 are skipped, 3 uses the current variance.
// Normalised rewards never feed back into the rollout, so the per-step semantics are computed after the fact over a whole
// time-major [T, N] block of raw rewards and dones, in three launches:
//   scan   one lane per env walks t = 0..T-1 with `returns` in an fp64 register; per t the wave's 64 returns are reduced by a
//          butterfly (fixed order) to one partial (mean, M2 = sum of squared deviations) in a [T, waves] workspace
//   merge  one workgroup: one wave per t combines the partials of that t (fixed lane assignment, fixed butterfly), then ONE lane runs
//          the T sequential merges into ret_rms; 1 / sqrt(var_t + eps) per t and the final (mean, var, count) are written
//   apply  out[t, n] = clip(float(double(r[t, n]) * inv_sigma[t])); in place allowed
// Properties the tests pin:
//   * no floating-point atomics, every reduction order is a function of N alone: results are bit-identical from run to run;
//   * the batch moments of step t are a function of returns[:, t] and N only -- not of T, of the position of t in the block or of where
//     the block starts -- and the sequential merges see them in the order of t: T calls of one step, one call of T steps and any other
//     split give the same bytes (outputs, statistics, carried returns);
//   * fp64 for the returns and the statistics (1 / sigma scales rewards in the hundreds: amenv_obsnorm.hpp on why fp64);
//   * lanes past N contribute exact zeros.
// Workspace: sized at create time for kRetnormChunk steps.  A longer block is neither refused nor does the workspace grow: the host walks
// it in consecutive chunks of at most kRetnormChunk steps (scan, merge, apply per chunk), which the chunking property makes invisible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amenv_dev {

constexpr int kRetnormChunk = 128;      // steps per scan / merge / apply round; the workspace holds this many rows of partials
constexpr int kRetnormMergeBlock = 1024;   // the merge workgroup: 16 waves, two t each per round
constexpr int kRetnormScanRows = 4;        // rows whose wave reductions the scan keeps in flight together

// device buffer of a handle (doubles): [0] mean | [1] var | [2] count | [3, 3 + chunk) inv_sigma | returns [N] | partials [chunk][waves][2]
__host__ __device__ inline int64_t retnorm_waves(int64_t n) { return (n + 63) / 64; }
__host__ __device__ inline int64_t retnorm_off_returns() { return 4 + kRetnormChunk; }   // even: the partials stay 16-byte aligned
__host__ __device__ inline int64_t retnorm_off_partials(int64_t n) { return retnorm_off_returns() + ((n + 1) & ~int64_t(1)); }
__host__ __device__ inline int64_t retnorm_words(int64_t n) { return retnorm_off_partials(n) + 2 * int64_t(kRetnormChunk) * retnorm_waves(n); }

// Steps 1 and 4 per env, and the wave's share of step 2.  Sums over the 64 lanes of a wave are butterflies (v += shfl_xor(v, 32), 16, .. 1):
// every lane gets the total and the order of the additions is fixed.  The partial of wave w at step t is (mean_w, M2_w) of its `cnt` valid returns,
// from sums of x - pivot and (x - pivot)^2 where pivot is the wave's first return: with a pivot taken from the data the cancellation in
// q - s^2 / cnt loses at most a factor cnt = 64 (the offset of 300 per step in the rewards, 3e4 in the returns, never enters a square).
__global__ __launch_bounds__(64) void retnorm_scan_kernel(const float* __restrict__ rewards, const uint8_t* __restrict__ dones, int T, int64_t N,
                                                          double gamma, double* __restrict__ returns, double* __restrict__ partials) {
  const int64_t wave = blockIdx.x, W = gridDim.x;
  const int64_t i = wave * 64 + threadIdx.x;
  const bool valid = i < N;
  const int64_t left = N - wave * 64;
  const double cnt = double(left < 64 ? left : 64), inv_cnt = 1.0 / cnt;   // 1 / 64 is exact for every full wave
  double ret = valid ? returns[i] : 0.0;
  // U rows per round: the recurrence is three operations per row, the butterflies are the latency, and those of U rows are independent
  constexpr int U = kRetnormScanRows;
  float r[U], r_n[U];
  uint8_t d[U], d_n[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const bool in = valid && u < T;
    r[u] = in ? rewards[int64_t(u) * N + i] : 0.0f;
    d[u] = in ? dones[int64_t(u) * N + i] : uint8_t(0);
  }
  for (int t0 = 0; t0 < T; t0 += U) {
#pragma unroll
    for (int u = 0; u < U; u++) {   // the next round's loads are in flight during this round's reductions
      const bool in = valid && t0 + U + u < T;
      r_n[u] = in ? rewards[int64_t(t0 + U + u) * N + i] : 0.0f;
      d_n[u] = in ? dones[int64_t(t0 + U + u) * N + i] : uint8_t(0);
    }
    double pivot[U], s[U], q[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (t0 + u < T) ret = ret * gamma + double(r[u]);   // rows past T (last round only) leave the carried return alone; their sums are not stored
      pivot[u] = __shfl(ret, 0, 64);                      // lane 0 is valid in every wave of the grid
      s[u] = valid ? ret - pivot[u] : 0.0;
      q[u] = s[u] * s[u];
      if (d[u]) ret = 0.0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int u = 0; u < U; u++) { s[u] += __shfl_xor(s[u], m, 64); q[u] += __shfl_xor(q[u], m, 64); }
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (t0 + u < T) {
          const double m2 = q[u] - s[u] * (s[u] * inv_cnt);
          double2 p;
          p.x = pivot[u] + s[u] * inv_cnt;
          p.y = m2 > 0.0 ? m2 : 0.0;
          *reinterpret_cast<double2*>(partials + 2 * (int64_t(t0 + u) * W + wave)) = p;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) { r[u] = r_n[u]; d[u] = d_n[u]; }
  }
  if (valid) returns[i] = ret;
}

// Step 2 for the T steps of a chunk, in the order of t, and 1 / sigma_t for step 3.
//   a. wave k of the workgroup takes t = k, k + 16, ...: lane l adds the partials of waves l, l + 64, ... in that order, a butterfly adds the
//      lanes: batch mean = sum(cnt_w mean_w) / N, batch var = sum(M2_w + cnt_w (mean_w - mean)^2) / N (np.var: population variance)
//   b. RunningMeanStd.update_from_moments (obsnorm_merge_kernel's formula) for t = 0..T-1.  count_t = count_{t-1} + N is a chain of
//      additions (rounded as numpy's); the two quotients of a merge, a = N / tot and c = count / tot, hang on the counts alone and are formed
//      for all t in parallel, so that the one sequential lane runs five dependent fp64 operations per step and no division:
//        mean' = mean + delta a ;  var' = (var count + b_var N + delta^2 count N / tot) / tot = var c + b_var a + delta^2 (c a)
//   c. inv_sigma[t] = 1 / sqrt(var_t + eps), parallel over t.
__global__ __launch_bounds__(kRetnormMergeBlock) void retnorm_merge_kernel(double* __restrict__ buf, int T, int64_t N, double eps) {
  __shared__ double b_mean[kRetnormChunk], b_var[kRetnormChunk], qa[kRetnormChunk], qc[kRetnormChunk];
  const double* partials = buf + retnorm_off_partials(N);
  const int64_t W = retnorm_waves(N);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double n = double(N);
  constexpr int kWaves = kRetnormMergeBlock / 64;
  for (int t0 = wave; t0 < T; t0 += 2 * kWaves) {   // two steps per round (t0 and t0 + 16): their butterflies are independent
    const double* row[2];
    double s[2], mean[2], m[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = t0 + u * kWaves;
      row[u] = partials + 2 * int64_t(t < T ? t : t0) * W;   // a step past T re-reads row t0 and is not stored
      s[u] = 0.0;
      for (int64_t w = lane; w < W; w += 64) {
        const int64_t left = N - w * 64;
        s[u] += double(left < 64 ? left : 64) * row[u][2 * w];
      }
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) { s[0] += __shfl_xor(s[0], mask, 64); s[1] += __shfl_xor(s[1], mask, 64); }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      mean[u] = s[u] / n;
      m[u] = 0.0;
      for (int64_t w = lane; w < W; w += 64) {
        const int64_t left = N - w * 64;
        const double dm = row[u][2 * w] - mean[u];
        m[u] += row[u][2 * w + 1] + double(left < 64 ? left : 64) * (dm * dm);
      }
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) { m[0] += __shfl_xor(m[0], mask, 64); m[1] += __shfl_xor(m[1], mask, 64); }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int t = t0 + u * kWaves;
        if (t < T) { b_mean[t] = mean[u]; b_var[t] = m[u] / n; }
      }
    }
  }
  if (threadIdx.x == 0) {
    double count = buf[2];
    for (int t = 0; t < T; t++) { qc[t] = count; count += n; }
    buf[2] = count;
  }
  __syncthreads();
  if (threadIdx.x < T) {
    const int t = threadIdx.x;
    const double count = qc[t], tot = count + n;
    const double a = n / tot, c = count / tot;
    qa[t] = a;
    qc[t] = c;
    b_var[t] = b_var[t] * a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double mean = buf[0], var = buf[1];
    for (int t = 0; t < T; t++) {
      const double delta = b_mean[t] - mean, a = qa[t], c = qc[t];
      mean = mean + delta * a;
      var = var * c + b_var[t] + (delta * delta) * (c * a);
      b_mean[t] = var;
    }
    buf[0] = mean;
    buf[1] = var;
  }
  __syncthreads();
  if (threadIdx.x < T) buf[3 + threadIdx.x] = 1.0 / sqrt(b_mean[threadIdx.x] + eps);
}

// Step 3: VecNormalize.normalize_reward.  Row t of the chunk is scaled with inv_sigma[t] (training) or, frozen, with the current variance.
// `in` and `out` may be the same buffer: an element is read and written by the same lane.
__global__ __launch_bounds__(256) void retnorm_apply_kernel(const float* in, float* out, int64_t N, const double* __restrict__ buf, int frozen,
                                                            float clip, double eps) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double inv_sigma = frozen ? 1.0 / sqrt(buf[1] + eps) : buf[3 + blockIdx.y];
  const int64_t e = int64_t(blockIdx.y) * N + i;
  float v = float(double(in[e]) * inv_sigma);
  v = v < -clip ? -clip : (v > clip ? clip : v);
  out[e] = v;
}

}  // namespace amenv_dev
