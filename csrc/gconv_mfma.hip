// Grouped 2-D implicit-GEMM convolution for gfx950 (MI355X): forward, data gradient and weight gradient of every
// group in one launch per direction, on v_mfma_f32_16x16x32_bf16.
//
// Reference: S/nn/SpatialConvolution.scala:253 (nGroup > 1: one im2col + gemm per group and sample).
//
//  * activations bf16 NHWC over ALL channels (x[N][H][W][C], dy[N][OH][OW][K]): a group's channels are contiguous, so
//    a tile of 64 output columns that spans the groups gA .. gB reads ONE contiguous channel range per tap,
//    [gA rg, (gB + 1) rg) with rg reduction channels per group; weights bf16 [K][R][S][cin_g] (forward, weight
//    gradient) or the per-group transpose [C][R][S][cout_g] (data gradient); fp32 accumulation;
//  * forward and data gradient share one "NT" kernel (the data gradient swaps the roles of C and K): 256 threads
//    (2 x 2 waves), a 128 x 64 or 64 x 64 tile, two 32-wide MFMA steps per 64-element LDS stage, register-staged
//    double-buffered LDS with the 2-D kernels' XOR slot swizzle. The reduction runs over (tap, channel of the tile's
//    range); a lane decodes its rows' pixels once and the tap of its granule arithmetically, so a stage may straddle
//    taps and kernel extents, strides and dilations are unbounded. A granule in the padding, past the reduction or
//    past the tile is staged as zeros with no load issued;
//  * what makes it grouped: the weight operand is staged block-diagonal (a column's granule is loaded only where the
//    granule's channels belong to the column's group, exact zeros elsewhere), and a 16-column MFMA block issues an
//    MFMA step only if one of the step's four granules lies in the channel range of the block's group(s). The stage's
//    granule channels sit in a small LDS table beside the operands. With columns-per-group a multiple of 16 every
//    block lies in one group and reduces over that group's channels alone; with a remainder of 8 a block straddles
//    two groups and reduces over both against the block-diagonal operand;
//  * the data gradient runs one dense pass per stride phase of the input grid (blockIdx.z) over the taps that reach
//    the phase (with dilation d: the taps kk with d kk = phase + pad mod stride); a phase without taps stores zeros;
//  * the weight gradient is a "TN" GEMM over the output pixels: a workgroup owns 64 output channels x one tap x a
//    64-channel chunk of the input channels of those output channels' groups and a contiguous pixel range, reads both
//    pixel-major operands from LDS with ds_read_b64_tr_b16, skips the 16 x 16 blocks whose input and output channels
//    share no group, stores only in-group elements as fp32 partials per pixel split, and bigdl_split_reduce_f32 adds
//    the splits in fixed order (no atomics anywhere: results are the same bits on every run).

// Device code without packed fp32 instructions, as csrc/conv3d.hip (see there): the bias add, the bias column sums
// and the epilogue are pinned bit for bit by the exact tests.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "lds_tr.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

// __syncthreads() spelled out so that it carries this file's target attribute and is inlined (see conv3d.hip)
__device__ __forceinline__ void wg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int BK = 64;   // reduction elements per LDS stage (8 granules per row, two MFMA steps)
constexpr int BN = 64;   // output columns per tile

// One axis (h or w) of an NT launch. GEMM rows walk e = 0 .. E-1 along it; tap j = 0 .. nj-1 (real kernel index
// k0 + j * kstep) reads source coordinate e * smul + soff + dir * j (valid inside [0, S)); the row lands at output
// coordinate e * omul + ooff of an axis of extent O.
struct Axis {
  int E, S, smul, soff, dir, nj, k0, kstep, O, omul, ooff;
};
__device__ __forceinline__ Axis fwd_axis(int in, int out, int k, int s, int p, int d) {
  return Axis{out, in, s, -p, d, k, 0, 1, out, 1, 0};
}
// input positions i = ph + s * e get dy[(i + p - d * kk) / s] * w[kk] for the kk with d * kk = ph + p (mod s): with
// q = gcd(d, s) these are k0, k0 + s / q, ... (none when q does not divide ph + p), and tap j reads dy at
// e + (ph + p - d * k0) / s - j * d / q
__device__ __forceinline__ Axis dgrad_axis(int in, int out, int k, int s, int p, int d, int ph) {
  int q = d, r = s;
  while (r) { const int t = q % r; q = r; r = t; }
  const int kstep = s / q;
  int k0 = -1;
  for (int kk = 0; kk < kstep && k0 < 0; ++kk)
    if ((ph + p - d * kk) % s == 0) k0 = kk;
  const bool any = k0 >= 0 && k0 < k;
  if (!any) k0 = 0;
  return Axis{ph < in ? (in - ph + s - 1) / s : 0, out, 1, any ? (ph + p - d * k0) / s : 0, -(d / q),
              any ? (k - k0 + kstep - 1) / kstep : 0, k0, kstep, in, s, ph};
}

struct NtArgs {
  const bf16_t* src;   // [N][Sh][Sw][Cs]
  const bf16_t* wt;    // [Ncol][R][S][Cs / G]
  const float* bias;   // [Ncol] or null
  void* out;           // [N][Oh][Ow][Ncol], bf16 or fp32
  GConvMfmaGeo g;
  int relu;
};

__device__ __forceinline__ int swz(int row, int g) { return row * BK + ((g ^ (row & 7)) << 3); }

template <int BM, bool DGRAD, bool OUT16>
__global__ __launch_bounds__(256, 2) void gconv_nt_kernel(NtArgs a) {
  constexpr int TM = BM / 2, TN = BN / 2;          // per-wave tile (2 x 2 waves)
  constexpr int MI = TM / 16, NI = TN / 16;
  constexpr int AROWS = BM / 32, BROWS = BN / 32;  // rows staged per thread
  constexpr int STAGE = (BM + BN) * BK;
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * STAGE];
  __shared__ __attribute__((aligned(16))) int gtab[2 * 8];   // per stage: first channel of each granule (-1: none)

  const GConvMfmaGeo& g = a.g;
  Axis xh, xw;
  int Cs, Ncol;
  if constexpr (DGRAD) {
    const int ph = blockIdx.z;
    xh = dgrad_axis(g.H, g.OH, g.R, g.sH, g.pH, g.dH, ph / g.sW);
    xw = dgrad_axis(g.W, g.OW, g.S, g.sW, g.pW, g.dW, ph % g.sW);
    Cs = g.K; Ncol = g.C;
  } else {
    xh = fwd_axis(g.H, g.OH, g.R, g.sH, g.pH, g.dH);
    xw = fwd_axis(g.W, g.OW, g.S, g.sW, g.pW, g.dW);
    Cs = g.C; Ncol = g.K;
  }
  const int ng = Ncol / g.G, rg = Cs / g.G;   // columns and reduction channels per group
  const int M = g.N * xh.E * xw.E;
  const int tiles_n = (Ncol + BN - 1) / BN, tiles_m = (M + BM - 1) / BM;
  if ((int)blockIdx.x >= tiles_m * tiles_n) return;   // a smaller phase than the grid was sized for
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;   // n fastest: neighbours share the A panel
  const int m0 = tm * BM, n0 = tn * BN;
  // the tile's groups and their channels: the reduction runs over (tap, channel cbase + c), c in [0, Wc)
  const int gA = n0 / ng, gB = min(n0 + BN - 1, Ncol - 1) / ng;
  const int cbase = gA * rg, Wc = (gB - gA + 1) * rg;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = tid >> 3, lg = tid & 7;

  // ---- this thread's A rows, decoded once ----
  int a_n[AROWS], a_h[AROWS], a_w[AROWS];
  const int ehw = xh.E * xw.E;
#pragma unroll
  for (int i = 0; i < AROWS; ++i) {
    const int m = m0 + lrow + 32 * i;
    if (m < M) {
      const int nb = m / ehw, r1 = m - nb * ehw;
      const int eh = r1 / xw.E, ew = r1 - eh * xw.E;
      a_n[i] = nb;
      a_h[i] = eh * xh.smul + xh.soff;
      a_w[i] = ew * xw.smul + xw.soff;
    } else {
      a_n[i] = 0; a_h[i] = -(1 << 28); a_w[i] = 0;   // never inside the source
    }
  }
  // ---- this thread's B rows (output columns): the column's group owns the channels [b_sub, b_sub + rg) of the range
  const int wtaps = g.R * g.S;
  long b_off[BROWS];
  int b_sub[BROWS];
#pragma unroll
  for (int i = 0; i < BROWS; ++i) {
    const int n = n0 + lrow + 32 * i;
    if (n < Ncol) {
      b_sub[i] = (n / ng - gA) * rg;
      b_off[i] = (long)n * wtaps * rg - b_sub[i];
    } else {
      b_sub[i] = -(1 << 28); b_off[i] = 0;   // never loaded
    }
  }

  // ---- this thread's granule: channel offset and tap (jh, jw), advanced by BK every stage ----
  const int ntaps = xh.nj * xw.nj;
  const int nk = (ntaps * Wc + BK - 1) / BK;
  int c = 0, jh = 0, jw = 0;
  if (ntaps > 0) {
    const int kk = lg * 8, tap = kk / Wc;
    c = kk - tap * Wc;
    jw = tap % xw.nj;
    jh = tap / xw.nj;
  }
  auto advance = [&]() {
    c += BK;
    while (c >= Wc) {
      c -= Wc;
      if (++jw == xw.nj) { jw = 0; ++jh; }
    }
  };

  v4u ra[AROWS], rb[BROWS];
  int rc = -1;
  auto gload = [&]() {
    const bool kvalid = jh < xh.nj;
    rc = kvalid ? c : -1;
    const int dh = xh.dir * jh, dw = xw.dir * jw;
    const int wtap = (xh.k0 + jh * xh.kstep) * g.S + xw.k0 + jw * xw.kstep;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
      const int sh = a_h[i] + dh, sw = a_w[i] + dw;
      ra[i] = v4u{0u, 0u, 0u, 0u};
      if (kvalid && (unsigned)sh < (unsigned)xh.S && (unsigned)sw < (unsigned)xw.S)
        ra[i] = *reinterpret_cast<const v4u*>(a.src + (((size_t)a_n[i] * xh.S + sh) * xw.S + sw) * Cs + cbase + c);
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      rb[i] = v4u{0u, 0u, 0u, 0u};
      if (kvalid && c >= b_sub[i] && c < b_sub[i] + rg)   // the granule's channels are the column's group's
        rb[i] = *reinterpret_cast<const v4u*>(a.wt + b_off[i] + (long)wtap * rg + c);
    }
  };
  auto swrite = [&](int buf) {
    bf16_t* A = lds + buf * STAGE;
    bf16_t* B = A + BM * BK;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) *reinterpret_cast<v4u*>(A + swz(lrow + 32 * i, lg)) = ra[i];
#pragma unroll
    for (int i = 0; i < BROWS; ++i) *reinterpret_cast<v4u*>(B + swz(lrow + 32 * i, lg)) = rb[i];
    if (tid < 8) gtab[buf * 8 + lg] = rc;   // lrow == 0, lg == tid
  };

  // the channel range [clo, chi) of the group(s) of each of this wave's 16-column blocks (empty past the columns)
  int clo[NI], chi[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int nb0 = n0 + wn * TN + j * 16;
    clo[j] = chi[j] = 0;
    if (nb0 < Ncol) {
      clo[j] = (nb0 / ng - gA) * rg;
      chi[j] = (min(nb0 + 15, Ncol - 1) / ng - gA + 1) * rg;
    }
  }

  v4f acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  if (nk > 0) {
    gload();
    swrite(0);
  }
  wg_sync();
  for (int ks = 0; ks < nk; ++ks) {
    const int cur = ks & 1;
    const bool more = ks + 1 < nk;
    if (more) {   // next stage's loads in flight during this stage's MFMAs
      advance();
      gload();
    }
    const bf16_t* A = lds + cur * STAGE;
    const bf16_t* B = A + BM * BK;
#pragma unroll
    for (int s = 0; s < BK / 32; ++s) {
      // which of the blocks have a granule of this step inside their groups' channels (uniform over the wave)
      const v4i t = *reinterpret_cast<const v4i*>(gtab + cur * 8 + s * 4);
      bool need[NI];
#pragma unroll
      for (int j = 0; j < NI; ++j) need[j] = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int tq = __builtin_amdgcn_readfirstlane(t[q]);
#pragma unroll
        for (int j = 0; j < NI; ++j) need[j] = need[j] || (tq >= clo[j] && tq < chi[j]);
      }
      bool any = false;
#pragma unroll
      for (int j = 0; j < NI; ++j) any = any || need[j];
      if (!any) continue;
      v8s fa[MI];
      const int gr = s * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const v8s*>(A + swz(wm * TM + i * 16 + (lane & 15), gr));
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        if (!need[j]) continue;
        const v8s fb = *reinterpret_cast<const v8s*>(B + swz(wn * TN + j * 16 + (lane & 15), gr));
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa[i], acc[i][j], 0, 0, 0);
      }
    }
    if (more) swrite(cur ^ 1);
    wg_sync();
  }

  // D[n][m] (weights were the MFMA A operand): the lane owns columns nb .. nb + 3 of row m = lane & 15; Ncol is a
  // multiple of 8, so the four columns are inside together: one 16-byte fp32 or 8-byte bf16 store along the channels
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = m0 + wm * TM + i * 16 + (lane & 15);
    if (m >= M) continue;
    size_t orow = m;
    if constexpr (DGRAD) {
      const int nb = m / ehw, r1 = m - nb * ehw;
      const int eh = r1 / xw.E, ew = r1 - eh * xw.E;
      orow = ((size_t)nb * xh.O + eh * xh.omul + xh.ooff) * xw.O + ew * xw.omul + xw.ooff;
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int nb = n0 + wn * TN + j * 16 + (lane >> 4) * 4;
      if (nb >= Ncol) continue;
      v4f v = acc[i][j];
      if (a.bias) v += *reinterpret_cast<const v4f*>(a.bias + nb);
      if (a.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      if constexpr (OUT16)
        *reinterpret_cast<v2u*>(static_cast<bf16_t*>(a.out) + orow * Ncol + nb) = v2u{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      else
        *reinterpret_cast<v4f*>(static_cast<float*>(a.out) + orow * Ncol + nb) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient: part[split][k][tap][c - group(k) cin_g] = sum over the split's pixels v of dy[v][k] * x[src(v, tap)][c]
// ------------------------------------------------------------------------------------------------
constexpr int WV = 64;   // pixels (reduction) per LDS stage
constexpr int WT = 64;   // tile: 64 k x 64 c

// [WV][64] bf16 image with the transposed-read slot function of conv3d.hip (8 rows -> 8 distinct bank groups)
__device__ __forceinline__ int wsw(int row, int col) {
  const int f = (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1;
  return row * WT + (((col >> 3) ^ f) << 3) + (col & 7);
}

struct WgArgs {
  const bf16_t* dy;   // [M][K]
  const bf16_t* x;    // [N][H][W][C]
  float* ws;          // [nsplit][K][taps][cin_g]
  float* wsb;         // [nsplit][K] or null
  GConvMfmaGeo g;
  int vper;           // pixels per split (a multiple of WV)
  int tiles_c;        // 64-channel chunks of the widest k tile's channel range
  int dn, dh, dw;     // WV pixels as a mixed-radix step over (n, oh, ow)
};

__global__ __launch_bounds__(256, 2) void gconv_wgrad_kernel(WgArgs a) {
  constexpr int STAGE = 2 * WV * WT;
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * STAGE];

  const GConvMfmaGeo& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 1, wk = wave & 1;   // wave tile: 32 c x 32 k
  const int taps = g.R * g.S, cin_g = g.C / g.G, cout_g = g.K / g.G;
  const int ct = blockIdx.x % a.tiles_c;
  const int tap = (blockIdx.x / a.tiles_c) % taps;
  const int k0 = (int)(blockIdx.x / (a.tiles_c * taps)) * WT;
  // the groups of this k tile and their input channels [cbase, cbase + Wc); this workgroup's chunk starts at c0
  const int gA = k0 / cout_g, gB = min(k0 + WT - 1, g.K - 1) / cout_g;
  const int cbase = gA * cin_g, Wc = (gB - gA + 1) * cin_g;
  const int c0 = ct * WT;
  if (c0 >= Wc) return;   // a narrower range than the grid was sized for (never chunk 0)
  const int kw = tap % g.S, kh = tap / g.S;
  const int M = g.N * g.OH * g.OW;
  const int vbeg = blockIdx.y * a.vper, vend = min(M, vbeg + a.vper);

  // loader: rows lrow and lrow + 32 of a stage, granule lg of both operands
  const int lrow = tid >> 3, lg = tid & 7;
  const bool kvalid = k0 + lg * 8 < g.K, cvalid = c0 + lg * 8 < Wc;
  int rn[2], rh[2], rw[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int v = vbeg + lrow + 32 * i;
    rw[i] = v % g.OW; v /= g.OW;
    rh[i] = v % g.OH; rn[i] = v / g.OH;
  }
  const bool do_bias = a.wsb != nullptr && tap == 0 && ct == 0;
  float bsum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bsum[e] = 0.f;

  v4u rdy[2], rx[2];
  auto gload = [&](int vb) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int v = vb + lrow + 32 * i;
      const int ih = rh[i] * g.sH - g.pH + kh * g.dH, iw = rw[i] * g.sW - g.pW + kw * g.dW;
      rdy[i] = v4u{0u, 0u, 0u, 0u};
      rx[i] = v4u{0u, 0u, 0u, 0u};
      if (v < vend) {
        if (kvalid) rdy[i] = *reinterpret_cast<const v4u*>(a.dy + (size_t)v * g.K + k0 + lg * 8);
        if (cvalid && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
          rx[i] = *reinterpret_cast<const v4u*>(a.x + (((size_t)rn[i] * g.H + ih) * g.W + iw) * g.C + cbase + c0 + lg * 8);
      }
      // step this row WV pixels on (each digit carries at most once)
      rw[i] += a.dw; if (rw[i] >= g.OW) { rw[i] -= g.OW; ++rh[i]; }
      rh[i] += a.dh; if (rh[i] >= g.OH) { rh[i] -= g.OH; ++rn[i]; }
      rn[i] += a.dn;
    }
  };
  auto swrite = [&](int buf) {
    bf16_t* D = lds + buf * STAGE;
    bf16_t* X = D + WV * WT;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = lrow + 32 * i;
      *reinterpret_cast<v4u*>(D + wsw(row, lg * 8)) = rdy[i];
      *reinterpret_cast<v4u*>(X + wsw(row, lg * 8)) = rx[i];
      if (do_bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { bsum[2 * e] += lo_bf(rdy[i][e]); bsum[2 * e + 1] += hi_bf(rdy[i][e]); }
      }
    }
  };

  // a 16 c x 16 k block is computed only if its input and its output channels share a group (uniform over the wave)
  bool need[2][2], need_x[2], need_d[2] = {false, false};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cb0 = c0 + wc * 32 + i * 16;
    need_x[i] = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kb0 = k0 + wk * 32 + j * 16;
      need[i][j] = false;
      if (cb0 < Wc && kb0 < g.K) {
        const int gc_lo = gA + cb0 / cin_g, gc_hi = gA + min(cb0 + 15, Wc - 1) / cin_g;
        const int gk_lo = kb0 / cout_g, gk_hi = min(kb0 + 15, g.K - 1) / cout_g;
        need[i][j] = gc_lo <= gk_hi && gk_lo <= gc_hi;
      }
      need_x[i] = need_x[i] || need[i][j];
      need_d[j] = need_d[j] || need[i][j];
    }
  }

  v4f acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  // transposed-read lane geometry (ds_read_b64_tr_b16): lane 4q + p of a 16-lane group addresses row q, columns
  // 4p .. 4p + 3 of a 4 x 16 block; lane i receives column i of the 4 rows
  const int G4 = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;

  gload(vbeg);
  swrite(0);
  wg_sync();
  int cur = 0;
  for (int vb = vbeg; vb < vend; vb += WV) {
    const bool more = vb + WV < vend;
    if (more) gload(vb + WV);
    const bf16_t* D = lds + cur * STAGE;
    const bf16_t* X = D + WV * WT;
#pragma unroll
    for (int s = 0; s < WV / 32; ++s) {
      v8s fx[2], fd[2];
      const int rbase = s * 32 + 8 * G4 + q;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (!need_x[i]) continue;
        const int col = wc * 32 + i * 16 + 4 * p;
        fx[i] = tr_join(__builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(v4s))(X + wsw(rbase, col))),
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(v4s))(X + wsw(rbase + 4, col))));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!need_d[j]) continue;
        const int col = wk * 32 + j * 16 + 4 * p;
        fd[j] = tr_join(__builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(v4s))(D + wsw(rbase, col))),
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(v4s))(D + wsw(rbase + 4, col))));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (need[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[i], fd[j], acc[i][j], 0, 0, 0);
    }
    if (more) swrite(cur ^ 1);
    wg_sync();
    cur ^= 1;
  }

  // D[c][k]: the lane holds c = cb .. cb + 3 (of the range) for k = lane & 15; cin_g is a multiple of 8, so the four
  // are in one group: one 16-byte store if that group is k's
  float* part = a.ws + (size_t)blockIdx.y * g.K * taps * cin_g;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cb = c0 + wc * 32 + i * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk * 32 + j * 16 + (lane & 15);
      if (!need[i][j] || k >= g.K || cb >= Wc) continue;
      const int cl = cb - (k / cout_g - gA) * cin_g;
      if (cl >= 0 && cl < cin_g) *reinterpret_cast<v4f*>(part + ((size_t)k * taps + tap) * cin_g + cl) = acc[i][j];
    }
  }
  if (do_bias) {   // column sums of this workgroup's dy rows: 32 row groups per granule, summed in row-group order
    float* red = reinterpret_cast<float*>(lds);   // the last barrier of the loop retired every LDS read
#pragma unroll
    for (int e = 0; e < 8; ++e) red[e * 256 + tid] = bsum[e];
    wg_sync();
    if (tid < 64) {
      const int gg = tid >> 3, e = tid & 7;
      float tot = 0.f;
      for (int rg = 0; rg < 32; ++rg) tot += red[e * 256 + rg * 8 + gg];
      const int k = k0 + gg * 8 + e;
      if (k < g.K) a.wsb[(size_t)blockIdx.y * g.K + k] = tot;
    }
  }
}

constexpr long LIM = 1l << 31;
constexpr int FILL_WGS = 512;        // workgroups that fill the chip (256 CUs x 2 resident)
constexpr int MIN_SPLIT_PIX = 256;   // a pixel split is at least this long (4 stages)

bool geo_ok(const GConvMfmaGeo* g) {
  if (g->N < 1 || g->H < 1 || g->W < 1 || g->OH < 1 || g->OW < 1 || g->C < 1 || g->K < 1) return false;
  if (g->G < 2 || g->C % g->G || g->K % g->G || ((g->C / g->G) & 7) || ((g->K / g->G) & 7)) return false;
  if (g->R < 1 || g->S < 1 || g->sH < 1 || g->sW < 1 || g->dH < 1 || g->dW < 1) return false;
  const long eh = (long)g->dH * (g->R - 1) + 1, ew = (long)g->dW * (g->S - 1) + 1;   // dilated kernel extents
  if (g->pH < 0 || g->pW < 0 || g->pH >= eh || g->pW >= ew) return false;
  if (g->H + 2l * g->pH < eh || g->W + 2l * g->pW < ew) return false;
  if ((g->H + 2l * g->pH - eh) / g->sH + 1 != g->OH || (g->W + 2l * g->pW - ew) / g->sW + 1 != g->OW) return false;
  if ((long)g->N * g->H * g->W * g->C >= LIM || (long)g->N * g->OH * g->OW * g->K >= LIM) return false;
  if ((long)g->R * g->S * (g->C / g->G) * g->K >= LIM || (long)g->sH * g->sW > 65535) return false;   // phases ride grid.z
  return true;
}

// 64-channel chunks of the widest channel range of a 64-column k tile: a tile touches at most 63 / cout_g + 2 groups
int wgrad_tiles_c(const GConvMfmaGeo* g) {
  const long groups = std::min<long>(g->G, (WT - 1) / (g->K / g->G) + 2);
  return (int)((groups * (g->C / g->G) + WT - 1) / WT);
}

// Number of pixel splits of the weight gradient and the pixels per split (a multiple of WV; no split is empty):
// enough splits to fill the chip, each at least MIN_SPLIT_PIX long.
int split_plan(const GConvMfmaGeo* g, int* vper_out) {
  const long M = (long)g->N * g->OH * g->OW;
  const long tiles = (long)((g->K + WT - 1) / WT) * g->R * g->S * wgrad_tiles_c(g);
  long want = FILL_WGS / tiles;
  if (want > M / MIN_SPLIT_PIX) want = M / MIN_SPLIT_PIX;
  if (want < 1) want = 1;
  const long vper = ((M + want - 1) / want + WV - 1) / WV * WV;
  if (vper_out) *vper_out = (int)vper;
  return (int)((M + vper - 1) / vper);
}

template <bool DGRAD>
int launch_nt(const NtArgs& a, long M, int Ncol, int phases, int out_bf16, hipStream_t st) {
  const int tiles_n = (Ncol + BN - 1) / BN;
  // 128-row tiles unless they leave the chip short of workgroups (small M or few column tiles)
  const bool small = ((M + 127) / 128) * tiles_n * phases < FILL_WGS / 2;
  const int bm = small ? 64 : 128;
  const long tiles = ((M + bm - 1) / bm) * tiles_n;
  if (tiles >= LIM) return -1;
  const dim3 grid((unsigned)tiles, 1, (unsigned)phases);
  if (small && out_bf16)
    hipLaunchKernelGGL((gconv_nt_kernel<64, DGRAD, true>), grid, dim3(256), 0, st, a);
  else if (small)
    hipLaunchKernelGGL((gconv_nt_kernel<64, DGRAD, false>), grid, dim3(256), 0, st, a);
  else if (out_bf16)
    hipLaunchKernelGGL((gconv_nt_kernel<128, DGRAD, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((gconv_nt_kernel<128, DGRAD, false>), grid, dim3(256), 0, st, a);
  HIP_LAUNCH_CHECK();
  return 0;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" {

int bigdl_gconv_mfma_supported(const GConvMfmaGeo* g) { return geo_ok(g) ? 1 : 0; }

int bigdl_gconv_mfma_fwd(const uint16_t* x, const uint16_t* w, const float* bias, void* y, int out_bf16, int relu,
                         const GConvMfmaGeo* g, hipStream_t st) {
  if (!geo_ok(g)) return -1;
  const NtArgs a{x, w, bias, y, *g, relu};
  return launch_nt<false>(a, (long)g->N * g->OH * g->OW, g->K, 1, out_bf16, st);
}

int bigdl_gconv_mfma_dgrad(const uint16_t* dy, const uint16_t* wt, void* dx, int out_bf16, const GConvMfmaGeo* g,
                           hipStream_t st) {
  if (!geo_ok(g)) return -1;
  const NtArgs a{dy, wt, nullptr, dx, *g, 0};
  // the grid is sized for phase (0, 0), the largest one
  const long M = (long)g->N * ((g->H + g->sH - 1) / g->sH) * ((g->W + g->sW - 1) / g->sW);
  return launch_nt<true>(a, M, g->C, g->sH * g->sW, out_bf16, st);
}

int bigdl_gconv_mfma_wgrad_splits(const GConvMfmaGeo* g) {
  if (!geo_ok(g)) return -1;
  return split_plan(g, nullptr);
}

int bigdl_gconv_mfma_wgrad_split_min(void) { return 2 * MIN_SPLIT_PIX; }

int bigdl_gconv_mfma_wgrad(const uint16_t* dy, const uint16_t* x, float* dw, float* db, float* ws,
                           const GConvMfmaGeo* g, hipStream_t st) {
  if (!geo_ok(g)) return -1;
  int vper = 0;
  const int nsplit = split_plan(g, &vper);
  const int taps = g->R * g->S;
  const long nw = (long)g->K * taps * (g->C / g->G);
  WgArgs a{dy, x, ws, db ? ws + nsplit * nw : nullptr, *g, vper, wgrad_tiles_c(g), 0, 0, 0};
  int r = WV;
  a.dw = r % g->OW; r /= g->OW;
  a.dh = r % g->OH; a.dn = r / g->OH;
  const long tiles = (long)((g->K + WT - 1) / WT) * taps * a.tiles_c;
  if (tiles >= LIM) return -1;
  hipLaunchKernelGGL(gconv_wgrad_kernel, dim3((unsigned)tiles, (unsigned)nsplit), dim3(256), 0, st, a);
  HIP_LAUNCH_CHECK();
  bigdl_split_reduce_f32(ws, dw, nw, db, g->K, nsplit, st);
  return 0;
}

}  // extern "C"
