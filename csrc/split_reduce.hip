// Sum of the weight-gradient split partials: dw[i] += sum over s of ws[s][i], for every split weight-gradient kernel
// (128 x 128 LDS-DMA, 256 x 256 phase-interleaved, 3x3 halo, stem) and, in the same launch, their bias partials.
//
// A workgroup of 256 threads owns cw = 2^cshift float4 columns and is rw = 256 / cw thread rows deep. Thread row g
// sums the splits g, g + rw, g + 2 rw, ... of its column in index order, eight independent 16-byte loads in flight per
// lane; row 0 then adds the rw row sums in row order out of LDS and adds the total into dw. The order depends on
// (n4, splits) alone and nothing is atomic, so the result is the same bits on every run. The partials are read once,
// so the kernel is as fast as the loads it keeps in flight: the launch picks cw so that even a 64 x 64 weight spreads
// over two workgroups per CU (narrow columns, deep rows), and a large weight reads 1 KB rows (cw = 64).
//
// The bias partials ([splits][nb4] float4 behind the dW partials) are one more column range: the workgroups from
// wblocks on sum them into dbias the same way.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int SR_LOADS = 8;

__global__ __launch_bounds__(256) void split_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, long n4,
                                                          const float* __restrict__ wsb, float* __restrict__ dbias,
                                                          long nb4, int wblocks, int splits, int cshift, int aligned) {
  __shared__ v4f red[256];
  const int cw = 1 << cshift, rw = 256 >> cshift;
  const int e = threadIdx.x & (cw - 1), g = threadIdx.x >> cshift;
  const bool bias = (int)blockIdx.x >= wblocks;
  const long n = bias ? nb4 : n4;
  const long i = (long)((int)blockIdx.x - (bias ? wblocks : 0)) * cw + e;
  v4f s = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    const v4f* p = reinterpret_cast<const v4f*>(bias ? wsb : ws) + (long)g * n + i;
    const long step = (long)rw * n;
    int sp = g;
#pragma unroll 1
    for (; sp + (SR_LOADS - 1) * rw < splits; sp += SR_LOADS * rw, p += SR_LOADS * step) {
      v4f a[SR_LOADS];
#pragma unroll
      for (int k = 0; k < SR_LOADS; ++k) a[k] = p[k * step];
#pragma unroll
      for (int k = 0; k < SR_LOADS; ++k) s += a[k];
    }
    // the last SR_LOADS - 1 splits at most: every load is issued (past the end it re-reads split 0 and adds zero), so
    // that none waits behind a branch on the one before
    const v4f* p0 = reinterpret_cast<const v4f*>(bias ? wsb : ws) + i;
    v4f a[SR_LOADS - 1];
#pragma unroll
    for (int k = 0; k < SR_LOADS - 1; ++k) a[k] = *(sp + k * rw < splits ? p + k * step : p0);
#pragma unroll
    for (int k = 0; k < SR_LOADS - 1; ++k) s += sp + k * rw < splits ? a[k] : v4f{0.f, 0.f, 0.f, 0.f};
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (g == 0 && i < n) {
    const int rows = min(rw, splits);
    v4f t = red[e];
#pragma unroll 8
    for (int r = 1; r < rows; ++r) t += red[(r << cshift) + e];
    float* o = (bias ? dbias : dw) + 4 * i;
    if ((aligned >> (bias ? 1 : 0)) & 1) {
      *reinterpret_cast<v4f*>(o) += t;
    } else {   // a view into a flat gradient buffer at a 4-byte-aligned offset
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] += t[k];
    }
  }
}

}  // namespace

extern "C" {

// dw[i] += sum over s of ws[s * n + i] and, with dbias, dbias[j] += sum over s of ws[splits * n + s * nb + j], in one
// launch and a fixed order (n % 4 == 0, nb % 4 == 0, ws 16-byte aligned).
void bigdl_split_reduce_f32(const float* ws, float* dw, long n, float* dbias, long nb, int splits, hipStream_t st) {
  const long n4 = n / 4, nb4 = dbias ? nb / 4 : 0;
  // the widest columns (<= 64 float4 = 1 KB rows) that still give two workgroups per CU
  const long want = 2L * conv_cus();
  int cshift = 6;
  while (cshift > 1 && (n4 >> cshift) < want) --cshift;
  const int cw = 1 << cshift;
  const int wblocks = (int)((n4 + cw - 1) / cw), bblocks = (int)((nb4 + cw - 1) / cw);
  const int aligned = ((reinterpret_cast<uintptr_t>(dw) & 15) == 0 ? 1 : 0) |
                      ((reinterpret_cast<uintptr_t>(dbias) & 15) == 0 ? 2 : 0);
  split_reduce_kernel<<<dim3((unsigned)(wblocks + bblocks)), dim3(256), 0, st>>>(
      ws, dw, n4, ws + (size_t)splits * n, dbias, nb4, wblocks, splits, cshift, aligned);
  HIP_LAUNCH_CHECK();
}

}  // extern "C"
