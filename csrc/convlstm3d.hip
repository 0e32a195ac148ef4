// Fused ConvLSTMPeephole3D steps for gfx950 (MI355X): one launch per time step and direction.
//
// Reference: S/nn/ConvLSTMPeephole3D.scala. The semantics are those of the 2-D step kernels (header of convlstm.hip):
// gate order i, f, g, o; peepholes pI, pF on c_{t-1} and pO on c_t (all three or none); tanh outside, sigmoid or
// hard-sigmoid inside (compile time); stride 1, odd cubic kernel k with zero "same" padding, C % 16 == 0; fp32 xg / c /
// gates / h, a bf16 copy of h, bf16 dg.
//
//   forward   pre = conv_same(h_{t-1}, U) + xg_t, then the cell      U  [4C][k][k][k][C]
//   backward  dh_t = dout_t + dh_T + conv_same(dg_{t+1}, U^T), ...   UT [C][k][k][k][4C], taps flipped on read
//
// Activations are dense channels-last [B, D, H, W, C]. The skeleton is the 2-D one with one more dimension:
//   * voxels live in a flat "virtual" space: every image row is followed by p = (k - 1) / 2 zero columns, every plane
//     by p zero rows and every volume by p zero planes (WP = W + p, HP = H + p, DP = D + p), all volumes of the batch
//     stacked. Tap (dd, dh, dw) of virtual voxel v is virtual voxel v + dd HP WP + dh WP + dw: a column, row or plane
//     past the volume lands on padding of the same or the neighbouring row / plane / volume (or before / after the
//     batch), which stages as zeros. A tile of TM consecutive virtual voxels may therefore span rows, planes and
//     volumes with no masks in the MFMA loop and nothing leaking across volumes.
//   * a workgroup owns TM = 64 virtual voxels x 64 output channels (4 waves = 4 channel fragments of 16). Per
//     32-channel chunk of the operand it stages, ONCE, the k^2 (plane, row) bands its taps touch: band (ddi, dhi) holds
//     virtual voxels v0 + (ddi - p) HP WP + (dhi - p) WP - p ... + TM + 2p at LDS row ddi * ps + dhi * ws.
//       ws = min(WP, TM + 2p): in a volume whose rows are shorter than a band the k row bands of one plane overlap in
//            the virtual space and collapse into one contiguous stretch of L = 2p ws + TM + 2p rows (nothing staged
//            twice); for longer rows they stay disjoint.
//       ps = HP WP if the row bands collapsed and HP WP < L, else L: plane stretches that overlap collapse the same
//            way into one run of 2p HP WP + L rows; otherwise they stay disjoint.
//     So R = 2p ps + L <= k^2 (TM + 2p) staged rows whatever D, H and W are. Tap (ddi, dhi, dwi) of tile voxel m is
//     LDS row ddi * ps + dhi * ws + dwi + m: a constant shift per tap. The row -> voxel map is decoded once per
//     workgroup into LDS; rows are 64 bytes with the granule swizzle of conv_halo.hip (conflict-free ds_read_b128 for
//     any row shift).
//   * K runs over taps x 32-channel chunks on v_mfma_f32_16x16x32_bf16, the weights as the first operand straight from
//     global memory (L2-resident, one tap ahead), the voxels as the second: a lane owns 4 consecutive channels of one
//     voxel. A 16-channel tail stages zero granules and loads zero weight fragments.
//   * forward: four gate accumulators per lane, the whole cell in registers; backward: one accumulator (4C operand
//     channels -> C), the cell backward in registers (convlstm_cell.h, shared with the 2-D kernels).
//
// LDS budget. A staged row costs 68 bytes (64 of operand, 4 of map). The 2-D tile of 128 voxels would need
// 9 x 130 x 68 = 79560 bytes for disjoint 3 x 3 x 3 bands, past the 64 KiB a launch gets by default. This file takes
// both steps the hardware offers:
//   * TM = 64: k = 3 needs at most 9 x 66 x 68 = 40392 bytes, k = 1 4352 bytes, inside the default limit for any D, H,
//     W. Four such workgroups fit the 160 KiB of a CU (more where bands collapse: 18768 bytes at 12 x 12 planes).
//   * the kernels' dynamic-LDS limit is raised to what the device grants a workgroup (160 KiB on gfx950, queried, never
//     assumed): k = 5 needs at most 25 x 68 x 68 = 115600 bytes and is served for any D, H, W at one workgroup per CU;
//     k = 7 (49 x 70 x 68 = 233240 bytes with every band disjoint) is served where bands collapse far enough for
//     R x 68 <= 160 KiB, i.e. R <= 2409: with collapsed rows and disjoint planes that is W <= 42.
// Anything larger returns -1 before a launch; nothing is launched with an LDS request the device would refuse.
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage); LDS is dynamic:
//   forward   116 VGPRs (112 with the hard-sigmoid) + 64 AGPRs, 64 SGPRs, no scratch: 2 waves per SIMD, so the
//             registers, not the LDS, bound the forward at 2 workgroups per CU
//   backward  70 VGPRs + 16 AGPRs, 58 SGPRs, no scratch: 5 waves per SIMD; the LDS bounds it at 4 workgroups per CU
//             for disjoint 3 x 3 x 3 bands
// k = 5 with disjoint bands and the served k = 7 tiles run one workgroup per CU (LDS).
//
// Peephole gradients: bigdl_convlstm_peep_wgrad of convlstm.hip over P = B D H W rows.

// Device code of this file is generated without packed fp32 instructions, as in convlstm.hip and conv3d.hip (see
// there); the attribute is pushed before the helper headers so that their inline functions carry it too.
#include <hip/hip_runtime.h>
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "common.h"
#include "kernels.h"
#include "convlstm_cell.h"

namespace {

using namespace convlstm_cell;

constexpr int TM = 64;         // virtual voxels per workgroup
constexpr int FM = TM / 16;    // voxel fragments per wave
constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_MAX = 160 * 1024;

struct Geo {
  int B, D, H, W, k;     // volumes, volume extent, kernel extent (odd)
  int p, DP, HP, WP;     // (k - 1) / 2, D + p, H + p, W + p
  int ws, ps, R;         // LDS row stride of a row band and of a plane stretch, staged rows
  long PS, V;            // virtual voxels of a plane HP * WP and of the batch B * DP * PS
};

Geo make_geo(int B, int D, int H, int W, int k) {
  Geo g;
  g.B = B; g.D = D; g.H = H; g.W = W; g.k = k;
  g.p = (k - 1) / 2; g.DP = D + g.p; g.HP = H + g.p; g.WP = W + g.p;
  const int band = TM + 2 * g.p;
  g.ws = g.WP < band ? g.WP : band;
  const int L = 2 * g.p * g.ws + band;
  g.PS = (long)g.HP * g.WP;
  g.ps = (g.ws == g.WP && g.PS < L) ? (int)g.PS : L;
  g.R = 2 * g.p * g.ps + L;
  g.V = (long)B * g.DP * g.PS;
  return g;
}
size_t lds_bytes(const Geo& g) { return (size_t)g.R * 64 + (size_t)g.R * 4; }

// Staged row -> voxel ((n * D + d) * H + i) * W + j, or -1 for padding and positions outside the batch.
__device__ __forceinline__ void decode_rows(const Geo& g, long v0, int* pix) {
  for (int r = threadIdx.x; r < g.R; r += 256) {
    int ddi = r / g.ps;
    if (ddi > 2 * g.p) ddi = 2 * g.p;
    const int r1 = r - ddi * g.ps;
    int dhi = r1 / g.ws;
    if (dhi > 2 * g.p) dhi = 2 * g.p;
    const long v = v0 + (long)(ddi - g.p) * g.PS + (long)(dhi - g.p) * g.WP - g.p + (r1 - dhi * g.ws);
    int P = -1;
    if (v >= 0 && v < g.V) {
      const long vr = v / g.WP;
      const int j = (int)(v - vr * g.WP);
      const long vp = vr / g.HP;
      const int i = (int)(vr - vp * g.HP);
      const int n = (int)(vp / g.DP), d = (int)(vp - (long)n * g.DP);
      if (j < g.W && i < g.H && d < g.D) P = ((n * g.D + d) * g.H + i) * g.W + j;
    }
    pix[r] = P;
  }
}

// acc[a][i] += sum over taps and operand channels of wrow[a][tap][c] * src[voxel of fragment i shifted by tap][c].
// src is [voxels][Cin] bf16; wrow[a] is this lane's weight row ([taps][Cin], already advanced by the lane's granule);
// flip reads tap (k^3 - 1 - tap) of the row (the transposed convolution). Every wave stages; only `active` waves (a
// channel fragment inside the tensor) load weights and multiply.
template <int NA>
__device__ __forceinline__ void halo_gemm(const Geo& g, const bf16_t* __restrict__ src, int Cin,
                                          const bf16_t* const (&wrow)[NA], bool flip, bool active, const int* pix,
                                          bf16_t* tile, v4f (&acc)[NA][FM]) {
  const int lane = threadIdx.x & 63, lg = lane >> 4;
  const int taps = g.k * g.k * g.k;
  const v8s zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int kc = 0; kc < Cin; kc += 32) {
    const bool kok = active && kc + 8 * lg < Cin;        // a 16-channel tail: granules 2, 3 are zeros on both sides
    v8s a[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) a[q] = kok ? ld8(wrow[q] + (long)(flip ? taps - 1 : 0) * Cin + kc) : zero;
    wg_sync();                                            // the previous chunk's fragment reads are done
    for (int e = threadIdx.x; e < g.R * 4; e += 256) {
      const int r = e >> 2, gr = e & 3;
      const int P = pix[r];
      v4u val = {0u, 0u, 0u, 0u};
      if (P >= 0 && kc + gr * 8 < Cin) val = *(const v4u*)(src + (long)P * Cin + kc + gr * 8);
      *(v4u*)(tile + r * 32 + ((gr ^ hswz(r)) << 3)) = val;
    }
    wg_sync();
    if (!active) continue;
    int tap = 0;
    for (int ddi = 0; ddi < g.k; ++ddi)
      for (int dhi = 0; dhi < g.k; ++dhi)
        for (int dwi = 0; dwi < g.k; ++dwi, ++tap) {
          v8s an[NA];
          const int nt = tap + 1 < taps ? tap + 1 : tap;  // next tap's weights are in flight during this tap's MFMAs
#pragma unroll
          for (int q = 0; q < NA; ++q) an[q] = kok ? ld8(wrow[q] + (long)(flip ? taps - 1 - nt : nt) * Cin + kc) : zero;
          const int r0 = ddi * g.ps + dhi * g.ws + dwi + (lane & 15);
          v8s b[FM];
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            const int r = r0 + 16 * i;
            b[i] = *(const v8s*)(tile + r * 32 + ((lg ^ hswz(r)) << 3));
          }
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int q = 0; q < NA; ++q) acc[q][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[q], b[i], acc[q][i], 0, 0, 0);
#pragma unroll
          for (int q = 0; q < NA; ++q) a[q] = an[q];
        }
  }
}

struct FwdArgs {
  const bf16_t* U;       // [4C][k][k][k][C]
  const bf16_t* h16;     // [P][C]     h_{t-1}
  const float* xg;       // [P][4C]    input projection of this step (bias included)
  const float* c_prev;   // [P][C]
  float* c_out;          // [P][C]
  bf16_t* h16_out;       // [P][C]
  float* h_out;          // [P][C]
  float* acts;           // [P][4C] post-activation gates, or null (inference)
  const float *pI, *pF, *pO;   // [C] each, or all null
  int C;
  Geo g;
};

template <bool HARD>
__global__ __launch_bounds__(256) void convlstm3d_fwd_step_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* tile = (bf16_t*)smem;
  int* pix = (int*)(smem + (size_t)a.g.R * 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4;
  const int C = a.C;
  const long v0 = (long)blockIdx.x * TM;
  const int cb = (blockIdx.y * 4 + wave) * 16;           // this wave's channel fragment
  const bool active = cb < C;
  decode_rows(a.g, v0, pix);
  const int taps = a.g.k * a.g.k * a.g.k;
  const bf16_t* wrow[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    wrow[q] = a.U + ((long)q * C + (active ? cb + (lane & 15) : 0)) * taps * C + 8 * lg;
  v4f acc[4][FM];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < FM; ++i) acc[q][i] = v4f{0.f, 0.f, 0.f, 0.f};
  halo_gemm<4>(a.g, a.h16, C, wrow, false, active, pix, tile, acc);
  if (!active) return;
  const int c4 = cb + 4 * lg;
  const bool peep = a.pI != nullptr;
  v4f wi = {0.f, 0.f, 0.f, 0.f}, wf = wi, wo = wi;
  if (peep) { wi = ld4f(a.pI + c4); wf = ld4f(a.pF + c4); wo = ld4f(a.pO + c4); }
  const int rc = a.g.p * (a.g.ps + a.g.ws + 1) + (lane & 15);   // the centre tap's row: the tile voxel itself
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int P = pix[rc + 16 * i];
    if (P < 0) continue;
    cell_fwd<HARD>(a, P, c4, peep, wi, wf, wo, acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
  }
}

struct BwdArgs {
  const bf16_t* UT;      // [C][k][k][k][4C]  (the transposed weight; taps are flipped on read)
  const bf16_t* dg_next; // [P][4C] dg_{t+1}, or null (last step)
  const float* dout;     // [P][C] or null
  const float* dh_ext;   // [P][C] or null (the gradient of h_T)
  const float* acts;     // [P][4C]
  const float* c_prev;   // [P][C]
  const float* c_t;      // [P][C]
  float* dc;             // [P][C] in: dc_t, out: dc_{t-1}
  bf16_t* dg_out;        // [P][4C]
  const float *pI, *pF, *pO;
  int C;
  Geo g;
};

template <bool HARD>
__global__ __launch_bounds__(256) void convlstm3d_bwd_step_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* tile = (bf16_t*)smem;
  int* pix = (int*)(smem + (size_t)a.g.R * 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4;
  const int C = a.C;
  const long v0 = (long)blockIdx.x * TM;
  const int cb = (blockIdx.y * 4 + wave) * 16;
  const bool active = cb < C;
  decode_rows(a.g, v0, pix);
  v4f acc[1][FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) acc[0][i] = v4f{0.f, 0.f, 0.f, 0.f};
  if (a.dg_next != nullptr) {
    const int taps = a.g.k * a.g.k * a.g.k;
    const bf16_t* wrow[1] = {a.UT + (long)(active ? cb + (lane & 15) : 0) * taps * 4 * C + 8 * lg};
    halo_gemm<1>(a.g, a.dg_next, 4 * C, wrow, true, active, pix, tile, acc);
  } else {
    wg_sync();                                           // pix is read below
  }
  if (!active) return;
  const int c4 = cb + 4 * lg;
  const bool peep = a.pI != nullptr;
  v4f wi = {0.f, 0.f, 0.f, 0.f}, wf = wi, wo = wi;
  if (peep) { wi = ld4f(a.pI + c4); wf = ld4f(a.pF + c4); wo = ld4f(a.pO + c4); }
  const int rc = a.g.p * (a.g.ps + a.g.ws + 1) + (lane & 15);
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int P = pix[rc + 16 * i];
    if (P < 0) continue;
    cell_bwd<HARD>(a, P, c4, peep, wi, wf, wo, acc[0][i]);
  }
}

bool shape_ok(int B, int C, int D, int H, int W, int k) {
  if (B <= 0 || C <= 0 || C % 16 != 0 || D <= 0 || H <= 0 || W <= 0 || k < 1 || k > 7 || k % 2 == 0) return false;
  const long p = (k - 1) / 2;
  // voxel indices are ints in the kernels; byte offsets are formed in 64 bits. The bound is checked factor by factor
  // so that the product itself cannot overflow.
  const long lim = (1l << 31) - 4 * TM;
  const long v1 = (long)B * (D + p);
  if (v1 >= lim) return false;
  const long v2 = v1 * (H + p);
  if (v2 >= lim) return false;
  return v2 * (W + p) < lim;
}

// What the device grants one workgroup: the opt-in limit where the runtime reports one, else the plain limit, never
// more than the 160 KiB this file was written for. One query per process (the devices of a host are alike).
size_t lds_cap() {
  static const size_t cap = [] {
    int dev = 0, optin = 0, plain = 0;
    if (hipGetDevice(&dev) != hipSuccess) return LDS_DEFAULT;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) optin = 0;
    if (hipDeviceGetAttribute(&plain, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) plain = 0;
    (void)hipGetLastError();
    const size_t v = (size_t)(optin > plain ? optin : plain);
    return v < LDS_DEFAULT ? LDS_DEFAULT : v > LDS_MAX ? LDS_MAX : v;
  }();
  return cap;
}

template <class K, class A>
int launch(K kernel, const A& a, int C, hipStream_t st) {
  const size_t lds = lds_bytes(a.g);
  if (lds > lds_cap()) return -1;
  if (lds > LDS_DEFAULT) {
    // only k >= 5 comes here; a runtime that refuses keeps the launch from happening
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_cap()) != hipSuccess) {
      (void)hipGetLastError();
      return -1;
    }
  }
  const dim3 grid((unsigned)((a.g.V + TM - 1) / TM), (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a);
  HIP_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int bigdl_convlstm3d_supported(int B, int C, int D, int H, int W, int k) {
  return shape_ok(B, C, D, H, W, k) && lds_bytes(make_geo(B, D, H, W, k)) <= lds_cap() ? 1 : 0;
}

int bigdl_convlstm3d_fwd_step(const uint16_t* U, const uint16_t* h16, const float* xg, const float* c_prev,
                              float* c_out, uint16_t* h16_out, float* h_out, float* acts, const float* pI,
                              const float* pF, const float* pO, int hard, int B, int C, int D, int H, int W, int k,
                              hipStream_t st) {
  if (!shape_ok(B, C, D, H, W, k)) return -1;
  if ((pI != nullptr) != (pF != nullptr) || (pI != nullptr) != (pO != nullptr)) return -1;
  const FwdArgs a{U, h16, xg, c_prev, c_out, h16_out, h_out, acts, pI, pF, pO, C, make_geo(B, D, H, W, k)};
  return hard ? launch(convlstm3d_fwd_step_kernel<true>, a, C, st) : launch(convlstm3d_fwd_step_kernel<false>, a, C, st);
}

int bigdl_convlstm3d_bwd_step(const uint16_t* UT, const uint16_t* dg_next, const float* dout, const float* dh_ext,
                              const float* acts, const float* c_prev, const float* c_t, float* dc, uint16_t* dg_out,
                              const float* pI, const float* pF, const float* pO, int hard, int B, int C, int D, int H,
                              int W, int k, hipStream_t st) {
  if (!shape_ok(B, C, D, H, W, k)) return -1;
  if ((pI != nullptr) != (pF != nullptr) || (pI != nullptr) != (pO != nullptr)) return -1;
  const BwdArgs a{UT, dg_next, dout, dh_ext, acts, c_prev, c_t, dc, dg_out, pI, pF, pO, C, make_geo(B, D, H, W, k)};
  return hard ? launch(convlstm3d_bwd_step_kernel<true>, a, C, st) : launch(convlstm3d_bwd_step_kernel<false>, a, C, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
