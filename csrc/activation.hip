// Point-wise activation layers (forward and backward) for gfx950: Tanh, Sigmoid, ELU, LeakyReLU, ReLU6, SoftPlus,
// SoftSign, HardTanh / Clamp, HardSigmoid, LogSigmoid, TanhShrink, SoftShrink, HardShrink, Threshold, Exp, Log,
// Sqrt, Square, Abs.
//
// Reference: the element-wise layers of S/nn/*.scala (Tanh.scala, Sigmoid.scala, ELU.scala, LeakyReLU.scala,
// ReLU6.scala, SoftPlus.scala, SoftSign.scala, HardTanh.scala, HardSigmoid.scala, LogSigmoid.scala,
// TanhShrink.scala, SoftShrink.scala, HardShrink.scala, Threshold.scala, Exp / Log / Sqrt / Square / Abs.scala)
// and the MKL VML calls behind them.
//
// One memory-bound pass each way: 16-byte vector loads (8 bf16 or 4 fp32 per lane), fp32 math, the activation kind
// is a wave-uniform argument (no divergence). Backward derivatives use the forward input x and / or output y, so
// no extra state is stored: dx = dy * f'(x, y).
#include "common.h"
#include "kernels.h"

namespace {

enum Act {
  A_TANH = 0, A_SIGMOID, A_ELU, A_LEAKY, A_RELU6, A_SOFTPLUS, A_SOFTSIGN, A_HARDTANH, A_HARDSIGMOID, A_LOGSIGMOID,
  A_TANHSHRINK, A_SOFTSHRINK, A_HARDSHRINK, A_THRESHOLD, A_EXP, A_LOG, A_SQRT, A_SQUARE, A_ABS
};

// The clamp-style kinds compare instead of fminf / fmaxf, so a NaN input stays a NaN (HardTanh.scala:93-97, the
// in-place form; Threshold.scala:83 x <= th ? v : x) and -0 inside the window keeps its sign.
__device__ __forceinline__ float act_f(int k, float x, float a, float b) {
  switch (k) {
    case A_TANH: return tanhf(x);
    case A_SIGMOID: return 1.f / (1.f + __expf(-x));
    case A_ELU: return x > 0.f ? x : a * (__expf(x) - 1.f);
    case A_LEAKY: return x > 0.f ? x : a * x;
    case A_RELU6: return x < 0.f ? 0.f : (x > 6.f ? 6.f : x);
    case A_SOFTPLUS: return x * a > 20.f ? x : log1pf(__expf(a * x)) / a;
    case A_SOFTSIGN: return x / (1.f + fabsf(x));
    case A_HARDTANH: return x < a ? a : (x > b ? b : x);
    case A_HARDSIGMOID: { const float t = 0.2f * x + 0.5f; return t < 0.f ? 0.f : (t > 1.f ? 1.f : t); }
    case A_LOGSIGMOID: return fminf(x, 0.f) - log1pf(__expf(-fabsf(x)));
    case A_TANHSHRINK: return x - tanhf(x);
    case A_SOFTSHRINK: return x > a ? x - a : (x < -a ? x + a : 0.f);
    case A_HARDSHRINK: return (x > a || x < -a) ? x : 0.f;
    case A_THRESHOLD: return x <= a ? b : x;
    case A_EXP: return __expf(x);
    case A_LOG: return __logf(x);
    case A_SQRT: return sqrtf(x);
    case A_SQUARE: return x * x;
    case A_ABS: return fabsf(x);
  }
  return x;
}

// derivative dy/dx from the input x and output y (clamp-style kinds pass the gradient on the closed interval,
// like the autograd reference)
__device__ __forceinline__ float act_df(int k, float x, float y, float a, float b) {
  switch (k) {
    case A_TANH: return 1.f - y * y;
    case A_SIGMOID: return y * (1.f - y);
    case A_ELU: return x > 0.f ? 1.f : y + a;
    case A_LEAKY: return x > 0.f ? 1.f : a;
    case A_RELU6: return (x >= 0.f && x <= 6.f) ? 1.f : 0.f;
    case A_SOFTPLUS: return x * a > 20.f ? 1.f : 1.f / (1.f + __expf(-a * x));
    case A_SOFTSIGN: { const float d = 1.f + fabsf(x); return 1.f / (d * d); }
    case A_HARDTANH: return (x >= a && x <= b) ? 1.f : 0.f;
    // decided in the x domain: 0.2*x+0.5 contracts to an FMA here, which would put the exact bf16 points
    // x = +-2.5 just outside the clamp window that the rounded-product reference keeps them in
    case A_HARDSIGMOID: return (x >= -2.5f && x <= 2.5f) ? 0.2f : 0.f;
    case A_LOGSIGMOID: return 1.f / (1.f + __expf(x));
    case A_TANHSHRINK: { const float t = tanhf(x); return t * t; }
    case A_SOFTSHRINK: return (x > a || x < -a) ? 1.f : 0.f;
    case A_HARDSHRINK: return (x > a || x < -a) ? 1.f : 0.f;
    case A_THRESHOLD: return x > a ? 1.f : 0.f;
    case A_EXP: return y;
    case A_LOG: return 1.f / x;
    case A_SQRT: return 0.5f / y;
    case A_SQUARE: return 2.f * x;
    case A_ABS: return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  }
  return 1.f;
}

template <bool BF>
__device__ __forceinline__ void ld8(const void* p, long i, float* v) {   // 8 elements at element index 8*i
  if constexpr (BF) {
    const v4u u = reinterpret_cast<const v4u*>(p)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = lo_bf(u[e]); v[2 * e + 1] = hi_bf(u[e]); }
  } else {
    const v4f a = reinterpret_cast<const v4f*>(p)[2 * i], b = reinterpret_cast<const v4f*>(p)[2 * i + 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
  }
}

template <bool BF>
__device__ __forceinline__ void st8(void* p, long i, const float* v) {
  if constexpr (BF) {
    reinterpret_cast<v4u*>(p)[i] = v4u{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]),
                                       pack2bf(v[6], v[7])};
  } else {
    reinterpret_cast<v4f*>(p)[2 * i] = v4f{v[0], v[1], v[2], v[3]};
    reinterpret_cast<v4f*>(p)[2 * i + 1] = v4f{v[4], v[5], v[6], v[7]};
  }
}

template <bool BF>
__device__ __forceinline__ float ld1(const void* p, long i) {
  if constexpr (BF) return bf2f(reinterpret_cast<const bf16_t*>(p)[i]);
  else return reinterpret_cast<const float*>(p)[i];
}

template <bool BF>
__device__ __forceinline__ void st1(void* p, long i, float v) {
  if constexpr (BF) reinterpret_cast<bf16_t*>(p)[i] = f2bf(v);
  else reinterpret_cast<float*>(p)[i] = v;
}

template <bool BF>
__global__ void act_fwd_kernel(const void* __restrict__ x, void* __restrict__ y, long n, long n8, int k, float a,
                               float b) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float v[8];
    ld8<BF>(x, i, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = act_f(k, v[e], a, b);
    st8<BF>(y, i, v);
  }
  for (long i = n8 * 8 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    st1<BF>(y, i, act_f(k, ld1<BF>(x, i), a, b));
}

template <bool BF>
__global__ void act_bwd_kernel(const void* __restrict__ x, const void* __restrict__ y, const void* __restrict__ dy,
                               void* __restrict__ dx, long n, long n8, int k, float a, float b) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float xv[8], yv[8], gv[8];
    ld8<BF>(x, i, xv);
    ld8<BF>(y, i, yv);
    ld8<BF>(dy, i, gv);
#pragma unroll
    for (int e = 0; e < 8; ++e) gv[e] *= act_df(k, xv[e], yv[e], a, b);
    st8<BF>(dx, i, gv);
  }
  for (long i = n8 * 8 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    st1<BF>(dx, i, ld1<BF>(dy, i) * act_df(k, ld1<BF>(x, i), ld1<BF>(y, i), a, b));
}

int blocks_for(long work) {
  long g = (work + 255) / 256;
  if (g > 8192) g = 8192;
  return g < 1 ? 1 : (int)g;
}

// 16-byte granules of the vector body: all of them when every pointer is 16-byte aligned, none otherwise (a view at an
// odd element offset inside a larger buffer then runs the scalar loop over the whole range)
template <typename... P>
long vec_granules(long n, P... ptrs) {
  return ((reinterpret_cast<uintptr_t>(ptrs) | ...) & 15) == 0 ? n >> 3 : 0;
}

}  // namespace

extern "C" {

int bigdl_act_fwd(const void* x, void* y, long n, int bf16, int kind, float a, float b, hipStream_t st) {
  if (kind < A_TANH || kind > A_ABS) return -1;
  const long n8 = vec_granules(n, x, y);
  const int g = blocks_for(n8 ? n8 : n);
  if (bf16) act_fwd_kernel<true><<<g, 256, 0, st>>>(x, y, n, n8, kind, a, b);
  else act_fwd_kernel<false><<<g, 256, 0, st>>>(x, y, n, n8, kind, a, b);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_act_bwd(const void* x, const void* y, const void* dy, void* dx, long n, int bf16, int kind, float a,
                  float b, hipStream_t st) {
  if (kind < A_TANH || kind > A_ABS) return -1;
  const long n8 = vec_granules(n, x, y, dy, dx);
  const int g = blocks_for(n8 ? n8 : n);
  if (bf16) act_bwd_kernel<true><<<g, 256, 0, st>>>(x, y, dy, dx, n, n8, kind, a, b);
  else act_bwd_kernel<false><<<g, 256, 0, st>>>(x, y, dy, dx, n, n8, kind, a, b);
  HIP_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
