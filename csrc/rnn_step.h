// Device helpers shared by the recurrent step kernels (csrc/lstm.hip, csrc/gru.hip, csrc/lstm_seq.hip): the gate
// non-linearities, the 16-byte bf16 fragment load, the K-split rule and the grouped-load MFMA loop.
#pragma once
#include "common.h"

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  const float e = __expf(-2.f * fabsf(x));
  const float t = (1.f - e) / (1.f + e);
  return x < 0.f ? -t : t;
}

__device__ __forceinline__ v8s ld8(const bf16_t* p) { return *(const v8s*)p; }

// K is consumed in groups of 8 k-steps whose loads are all issued before the group's MFMAs, so a wave pays about
// one memory round trip per group; the step kernels split K over many waves so that each wave has one or two groups
// (a long per-wave chain of L2/MALL round trips was the measured bottleneck, tools/lstm_micro.py).

// K-split factor: chunks of >= 256 (8 k-steps), at most `cap` waves per output tile.
__host__ __device__ inline int ksplit(int K, int cap) {
  int ks = K / 256;
  if (ks < 1) ks = 1;
  if (ks > cap) ks = cap;
  while (ks > 1 && (K % (ks * 32)) != 0) --ks;
  return ks;
}

// NS x NV output tiles: acc[i][n] += S[i] x V[n] (SFIRST: S is the MFMA's first operand) over K, every fragment
// loaded once per k-step and used by all the tiles of its row / column (NV = 2 halves the weight traffic per output).
template <int NS, int NV, bool SFIRST>
__device__ __forceinline__ void mfma_tiles(const bf16_t* const (&ps)[NS], const bf16_t* const (&pv)[NV], int K,
                                           v4f (&acc)[NS][NV]) {
  constexpr int CH = NS * NV > 2 ? 4 : 8;
  const int steps = K / 32, full = steps / CH * CH;
  for (int s = 0; s < full; s += CH) {
    v8s a[NS][CH], b[NV][CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
#pragma unroll
      for (int u = 0; u < NS; ++u) a[u][i] = ld8(ps[u] + (s + i) * 32);
#pragma unroll
      for (int n = 0; n < NV; ++n) b[n][i] = ld8(pv[n] + (s + i) * 32);
    }
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int u = 0; u < NS; ++u)
#pragma unroll
        for (int n = 0; n < NV; ++n)
          acc[u][n] = SFIRST ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][i], b[n][i], acc[u][n], 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n][i], a[u][i], acc[u][n], 0, 0, 0);
  }
  for (int s = full; s < steps; ++s) {
    v8s a[NS], b[NV];
#pragma unroll
    for (int u = 0; u < NS; ++u) a[u] = ld8(ps[u] + s * 32);
#pragma unroll
    for (int n = 0; n < NV; ++n) b[n] = ld8(pv[n] + s * 32);
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int n = 0; n < NV; ++n)
        acc[u][n] = SFIRST ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[n], acc[u][n], 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n], a[u], acc[u][n], 0, 0, 0);
  }
}
