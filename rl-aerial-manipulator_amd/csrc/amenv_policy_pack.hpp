// amenv_policy_pack.hpp -- policy_pack_kernel: the flat parameters of amenv_policy_mlp.hpp's network as the fragments its kernels consume.
// A non-template kernel: ONE source includes this header (amenv_capi.hip, policy_io), so that the library holds it once.
#pragma once
#include "amenv_policy_mlp.hpp"

namespace amenv_dev {

// fp32 parameters -> MFMA A-operand fragments (bf16) + bias quadruples, in the order the kernels' wavefronts consume them.
// One thread per (wavefront, item, lane); item < 18: fragment, else bias.  D, A: the caller's dimensions; pnj: see pol_in_col (the
// action rows 4 + pnj .. 6 of a shorter arm are zero: row < A below).
__global__ void policy_pack_kernel(const float* __restrict__ Pm, int D, int A, int pnj, uint32_t* __restrict__ out) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int per_wave = (kPolFrags + kPolBias) * 64;
  if (tid >= 4 * per_wave + 64 + 4 * 4 * 64) return;
  if (tid >= 4 * per_wave + 64) {   // second bf16 part of the first layer's weights, W1 - bf16(W1) (and of its bias column): fragment (wavefront w, tile j) at kPolLoBase + (4 w + j) * 64
    const int r = tid - (4 * per_wave + 64), w = r / 256, item = (r % 256) / 64, l = r & 63, row = l & 15, kq = l >> 4;
    const PolLayout Lo(D, A);
    const int T = 4 * w + item, net = T >> 3, neuron = 16 * (T & 7) + row;
    const float* W1 = Pm + (net == 0 ? Lo.o_pi : Lo.o_vf); const float* b1 = W1 + 128 * D;
    uint32_t o[4];
    for (int q = 0; q < 4; q++) {
      uint32_t two[2];
      for (int h = 0; h < 2; h++) {
        const int k = 8 * kq + 2 * q + h;
        const float v = pol_w1(W1, b1, neuron, k, D, pnj);
        two[h] = bf16_bits(v - float((__bf16)v));
      }
      o[q] = two[0] | (two[1] << 16);
    }
    uint32_t* dst = out + (size_t(kPolLoBase) + size_t(4 * w + item) * 64 + l) * 4;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3];
    return;
  }
  if (tid >= 4 * per_wave) {   // per-lane action constants: {std, log_std} of the wrench entry of lane c and of joint min(c, 2)
    const int l = tid - 4 * per_wave, cc = l & 3, cj = cc < 3 ? cc : 2;
    uint32_t* dst = out + size_t(4 * per_wave + l) * 4;
    dst[0] = __float_as_uint(expf(Pm[cc])); dst[1] = __float_as_uint(Pm[cc]);
    // (a rigid vehicle has no joint actions; a shorter arm's phantom joints have none either: zeros, nothing read past log_std[A - 1])
    dst[2] = 4 + cj < A ? __float_as_uint(expf(Pm[4 + cj])) : 0u; dst[3] = 4 + cj < A ? __float_as_uint(Pm[4 + cj]) : 0u;
    return;
  }
  const int w = tid / per_wave, item = (tid % per_wave) / 64, l = tid & 63;
  const PolLayout Lo(D, A);
  const int row = l & 15, kq = l >> 4;
  uint32_t o[4] = {0, 0, 0, 0};
  auto trunk_ptr = [&](int net) { return Pm + (net == 0 ? Lo.o_pi : Lo.o_vf); };
  if (item < kPolFrags) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = 0.0f;
    if (item < 4) {                                   // layer 1: combined tile 4w + item, K = D inputs + the bias column (obs column D = 1)
      const int T = 4 * w + item, net = T >> 3, neuron = 16 * (T & 7) + row;
      const float* W1 = trunk_ptr(net); const float* b1 = W1 + 128 * D;
      for (int j = 0; j < 8; j++) v[j] = pol_w1(W1, b1, neuron, 8 * kq + j, D, pnj);
    } else if (item < 12) {                           // layer 2: tile 2w + j, k-step ks
      const int j2 = (item - 4) >> 2, ks = (item - 4) & 3, T = 2 * w + j2, net = T >> 2, neuron = 16 * (T & 3) + row;
      const float* W2 = trunk_ptr(net) + 128 * D + 128;
      for (int j = 0; j < 8; j++) v[j] = W2[neuron * 128 + 32 * ks + 8 * kq + j];
    } else if (item < 16) {                           // layer 3
      const int j3 = (item - 12) >> 1, ks = (item - 12) & 1, T = 2 * w + j3, net = T >> 2, neuron = 16 * (T & 3) + row;
      const float* W3 = trunk_ptr(net) + 128 * D + 128 + 64 * 128 + 64;
      for (int j = 0; j < 8; j++) v[j] = W3[neuron * 64 + 32 * ks + 8 * kq + j];
    } else {                                          // heads: wavefront 0 the action mean (A rows), wavefront 1 the value (1 row)
      const int ks = item - 16;
      for (int j = 0; j < 8; j++) {
        const int k = 32 * ks + 8 * kq + j;
        v[j] = w == 0 ? (row < A ? Pm[Lo.o_actw + row * 64 + k] : 0.0f) : (w == 1 ? (row == 0 ? Pm[Lo.o_valw + k] : 0.0f) : 0.0f);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = bf16_bits(v[2 * q]) | (bf16_bits(v[2 * q + 1]) << 16);
  } else {                                            // biases of the D tile this lane accumulates: neurons 16 tile + 4 (l >> 4) + r
    const int bi = item - kPolFrags;
    float b[4] = {0, 0, 0, 0};
    for (int r = 0; r < 4; r++) {
      const int nn = 4 * kq + r;
      if (bi < 2) { const int T = 2 * w + bi, net = T >> 2; b[r] = (trunk_ptr(net) + 128 * D + 128 + 64 * 128)[16 * (T & 3) + nn]; }
      else if (bi < 4) { const int T = 2 * w + (bi - 2), net = T >> 2; b[r] = (trunk_ptr(net) + 128 * D + 128 + 64 * 128 + 64 + 64 * 64)[16 * (T & 3) + nn]; }
      else b[r] = w == 0 ? (nn < A ? Pm[Lo.o_actb + nn] : 0.0f) : (w == 1 ? (nn == 0 ? Pm[Lo.o_valb] : 0.0f) : 0.0f);
    }
    for (int q = 0; q < 4; q++) o[q] = __float_as_uint(b[q]);
  }
  uint32_t* dst = out + (size_t(w) * (kPolFrags + kPolBias) + item) * 64 * 4 + l * 4;
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3];
}

}  // namespace amenv_dev
