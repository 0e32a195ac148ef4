// What the fused ConvLSTMPeephole step kernels of convlstm.hip (2-D) and convlstm3d.hip (3-D) share: the LDS row
// swizzle, the workgroup barrier and the LSTM cell forward / backward of one (position, 4 channels) element held in
// registers. The cell functions are pure functions of registers and of the element's own rows of the step's buffers;
// `A` is the kernel's argument block (FwdArgs / BwdArgs of either file: same member names, channels-last rows).
//
// Include it inside the file's `no-packed-fp32-ops` attribute push: the functions must carry the attribute of the
// kernels they inline into.
#pragma once
#include "common.h"
#include "rnn_step.h"

namespace convlstm_cell {

__device__ __forceinline__ void wg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// granule slot swizzle of a 64-byte LDS row (conv_halo.hip): conflict-free 16-row fragment reads at any row offset
__device__ __forceinline__ int hswz(int r) { return ((r >> 2) & 1) << 1; }

template <bool HARD>
__device__ __forceinline__ float inner_act(float x) {
  if constexpr (HARD) return fminf(fmaxf(0.2f * x + 0.5f, 0.f), 1.f);
  else return sigm(x);
}
// derivative of the inner activation from its saved value
template <bool HARD>
__device__ __forceinline__ float inner_grad(float s) {
  if constexpr (HARD) return (s > 0.f && s < 1.f) ? 0.2f : 0.f;
  else return s * (1.f - s);
}

// bf16 bits -> fp32 by bit cast (the runtime header's __uint_as_float does not carry the files' target attribute
// and would stay a call)
__device__ __forceinline__ float bits_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ v4f ld4f(const float* p) { return *(const v4f*)p; }
__device__ __forceinline__ void st4bf(bf16_t* p, const v4f& v) {
  *(v2u*)p = v2u{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
}

// Forward cell of position P, channels c4 .. c4 + 3: pre[q] is the recurrent convolution's sum of gate block q.
template <bool HARD, class A>
__device__ __forceinline__ void cell_fwd(const A& a, int P, int c4, bool peep, const v4f& wi, const v4f& wf,
                                         const v4f& wo, const v4f& pi, const v4f& pf, const v4f& pg, const v4f& po) {
  const int C = a.C;
  const long pc = (long)P * C + c4, pg4 = (long)P * 4 * C + c4;
  const v4f xi = ld4f(a.xg + pg4), xf = ld4f(a.xg + pg4 + C), xc = ld4f(a.xg + pg4 + 2 * C), xo = ld4f(a.xg + pg4 + 3 * C);
  const v4f cp = ld4f(a.c_prev + pc);
  v4f gi, gf, gg, go, c, h;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float ai = pi[e] + xi[e], af = pf[e] + xf[e];
    if (peep) { ai += wi[e] * cp[e]; af += wf[e] * cp[e]; }
    gi[e] = inner_act<HARD>(ai);
    gf[e] = inner_act<HARD>(af);
    gg[e] = tanh_f(pg[e] + xc[e]);
    c[e] = gf[e] * cp[e] + gi[e] * gg[e];
    float ao = po[e] + xo[e];
    if (peep) ao += wo[e] * c[e];
    go[e] = inner_act<HARD>(ao);
    h[e] = go[e] * tanh_f(c[e]);
  }
  *(v4f*)(a.c_out + pc) = c;
  *(v4f*)(a.h_out + pc) = h;
  st4bf(a.h16_out + pc, h);
  if (a.acts != nullptr) {
    *(v4f*)(a.acts + pg4) = gi; *(v4f*)(a.acts + pg4 + C) = gf;
    *(v4f*)(a.acts + pg4 + 2 * C) = gg; *(v4f*)(a.acts + pg4 + 3 * C) = go;
  }
}

// Backward cell of position P, channels c4 .. c4 + 3: rec is the recurrent term conv(dg_{t+1}, U^T) of dh_t.
template <bool HARD, class A>
__device__ __forceinline__ void cell_bwd(const A& a, int P, int c4, bool peep, const v4f& wi, const v4f& wf,
                                         const v4f& wo, const v4f& rec) {
  const int C = a.C;
  const long pc = (long)P * C + c4, pg = (long)P * 4 * C + c4;
  const v4f ig = ld4f(a.acts + pg), fg = ld4f(a.acts + pg + C), gg = ld4f(a.acts + pg + 2 * C), og = ld4f(a.acts + pg + 3 * C);
  const v4f ct = ld4f(a.c_t + pc), cp = ld4f(a.c_prev + pc), dcn = ld4f(a.dc + pc);
  v4f dh = rec;
  if (a.dout != nullptr) { const v4f d = ld4f(a.dout + pc); dh += d; }
  if (a.dh_ext != nullptr) { const v4f d = ld4f(a.dh_ext + pc); dh += d; }
  v4f di, df, dgg, dog, dcp;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float tc = tanh_f(ct[e]);
    dog[e] = dh[e] * tc * inner_grad<HARD>(og[e]);
    float dcv = dh[e] * og[e] * (1.f - tc * tc) + dcn[e];
    if (peep) dcv += dog[e] * wo[e];
    di[e] = dcv * gg[e] * inner_grad<HARD>(ig[e]);
    df[e] = dcv * cp[e] * inner_grad<HARD>(fg[e]);
    dgg[e] = dcv * ig[e] * (1.f - gg[e] * gg[e]);
    dcp[e] = dcv * fg[e];
    if (peep) dcp[e] += di[e] * wi[e] + df[e] * wf[e];
  }
  *(v4f*)(a.dc + pc) = dcp;
  st4bf(a.dg_out + pg, di); st4bf(a.dg_out + pg + C, df);
  st4bf(a.dg_out + pg + 2 * C, dgg); st4bf(a.dg_out + pg + 3 * C, dog);
}

}  // namespace convlstm_cell
