// Fused depthwise-separable convolution forward for gfx950 (MI355X): ONE launch, the depthwise result never in HBM.
//
// Reference: S/nn/SpatialSeparableConvolution.scala:54 (depthwise kH x kW with depth multiplier dm, then 1 x 1).
//
//   mid[n][m][oh][ow] = sum_{r,s} wd[m][r][s] * x[n][m / dm][oh sH - pH + r][ow sW - pW + s]      (fp32, VALU)
//   y[n][k][oh][ow]   = bias[k] + sum_m wp[k][m] * (hi + lo)(mid[n][m][oh][ow])                   (bf16 MFMA, fp32 sum)
//   hi = bf16(mid), lo = bf16(mid - hi): mid enters the GEMM as two bf16 terms, 16 significant bits. One bf16 rounding
//   costs up to 2^-8 |mid| (8 significant bits), twice what the forward's error bound of 2^-9 allows; hi alone is what
//   mid16 holds.
//
// The two-kernel path writes mid to HBM in fp32, reads it back, writes it again as bf16 NHWC and reads that: here a
// workgroup computes the mid values of its pixel tile in LDS and consumes them at once as the B operand of the
// pointwise GEMM on v_mfma_f32_16x16x32_bf16.
//
//   * work split: a workgroup of 256 threads (4 waves) owns one image, TH x TW = 128 output pixels (8 x 16, or 16 x 8
//     for maps at most 8 wide) and BN = 64 NA output channels (NA = 1, 2, 4 channel fragments per wave, from Cout);
//     grid = (pixel tiles, Cout blocks, N). It loops over the mid channels in chunks of 32, the MFMA K.
//   * x halo: per chunk the ((TH-1) sH + kH) x ((TW-1) sW + kW) fp32 window of the chunk's input channels (mid channels
//     32 c .. 32 c + 31 read input channels (32 c) / dm .. (32 c + 31) / dm) goes global -> LDS by LDS-DMA dwords,
//     lanes along W of NCHW. The loads go through a buffer resource over the image; taps outside the image, channels
//     the chunk does not read and the round-up of the window are given an out-of-range offset and arrive as zeros. Two
//     windows are resident: chunk i + 2 is in flight while chunk i multiplies and chunk i + 1 is filtered.
//   * depthwise: wave w owns granule w (8 mid channels) of the chunk, a lane two pixels (lane, lane + 64): 16 fp32 sums
//     per thread, x from LDS (lanes along W), the chunk's weights from LDS too (staged with x, broadcast reads).
//     Each sum is rounded with f2bf to its high part, and the exact fp32 remainder to its low part; a lane's 8 channels
//     are one 16-byte store into each of the two [128][32] bf16 mid tiles, rows of 64 bytes with the granule swizzle of
//     conv_halo.hip (conflict-free 8-bf16 fragment reads). Pixels past OH / OW and channels past Cmid are stored as
//     zeros, so the GEMM has no tail case. The mid tiles are single: two barriers a chunk, LDS as for one bf16 pair.
//   * pointwise: A = 16 rows of the bf16 point weight [Cout8][Cmid32] per fragment, straight from global memory (L2-
//     resident, the same for every tile, one chunk ahead), B = the high, then the low mid tile. D is [out channel][pixel]: a lane holds 4
//     consecutive channels of pixel (lane & 15) of a fragment, so 16 lanes store 16 consecutive pixels of a row of one
//     channel, one 64-byte segment of fp32 NCHW. 8 NA accumulators (v4f) stay in registers over all chunks.
//   * epilogue: + fp32 bias, fp32 NCHW stores. Training also wants the bf16 NHWC mid tensor for the pointwise weight
//     gradient: Cout block 0 of every tile writes its high mid granules to mid16 as it goes (inference: null).
//
// No atomics, no scratch. The tap loops have runtime bounds on purpose: with compile-time 3 x 3 taps the compiler
// hoists all 144 LDS addresses of a chunk out of the chunk loop and the kernel spills.
#include "common.h"
#include "kernels.h"
#include "convlstm_cell.h"

namespace {

using convlstm_cell::hswz;
using convlstm_cell::wg_sync;

constexpr int TM = 128;                       // pixels per workgroup
constexpr int FM = TM / 16;                   // pixel fragments
constexpr int MID_BYTES = TM * 64;            // one [128][32] bf16 mid tile
constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_MAX = 160 * 1024;
constexpr unsigned OOB = 0x80000000u;         // buffer offset past any image: the load returns 0

struct Args {
  const float* x; const float* wd; const bf16_t* wp; const float* bias; float* y; bf16_t* mid16;
  int N, Cin, dm, H, W, Cout, OH, OW, kH, kW, sH, sW, pH, pW;
  int Cmid, Cmid8, Cmid32, Cout8;
  int HH, HW, plane, tilesW;                  // halo window extents, HH * HW
  int welems, xelems;                         // floats of a stage buffer's weights / x window (multiples of 256)
  unsigned mplane, mrow;                      // 2^32 / plane + 1, 2^32 / HW + 1: exact quotients for e < xelems
};

__device__ __forceinline__ v8s ld8(const bf16_t* p) { return *(const v8s*)p; }

// LDS-DMA of chunk kc's operands into one stage buffer, one dword per lane: the chunk's 32 x kH x kW depthwise weights
// (rows past Cmid lie past the buffer's end and arrive as zeros), then its x window, element e = (c, hy, hx) of
// [channels][HH][HW].
__device__ __forceinline__ void stage(const Args& a, const __amdgpu_buffer_rsrc_t& rx, const __amdgpu_buffer_rsrc_t& rw,
                                      int kc, float* buf, int wave, int lane, int ih0, int iw0) {
  const int w0 = kc * 32 * a.kH * a.kW;
  for (int e0 = wave * 64; e0 < a.welems; e0 += 256)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (LDS_PTR(void))(buf + e0), 4, (w0 + e0 + lane) * 4, 0, 0, 0);
  float* xs = buf + a.welems;
  const int c_lo = kc * 32 / a.dm;
  const int m_hi = kc * 32 + 31 < a.Cmid ? kc * 32 + 31 : a.Cmid - 1;
  const int nci = m_hi / a.dm - c_lo + 1;
  for (int e0 = wave * 64; e0 < a.xelems; e0 += 256) {
    const unsigned e = (unsigned)(e0 + lane);
    const unsigned c = __umulhi(e, a.mplane);
    const unsigned rem = e - c * (unsigned)a.plane;
    const unsigned hy = __umulhi(rem, a.mrow);
    const unsigned hx = rem - hy * (unsigned)a.HW;
    const int ih = ih0 + (int)hy, iw = iw0 + (int)hx;
    const bool ok = (int)c < nci && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
    const unsigned off =
        ok ? ((((unsigned)c_lo + c) * (unsigned)a.H + (unsigned)ih) * (unsigned)a.W + (unsigned)iw) * 4u : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (LDS_PTR(void))(xs + e0), 4, (int)off, 0, 0, 0);
  }
}

// Depthwise sums of chunk kc for this wave's granule and this lane's two pixels, rounded into the mid tile (and mid16).
template <int TW>
__device__ __forceinline__ void depthwise(const Args& a, int kc, const float* buf, bf16_t* mid, bf16_t* mid16,
                                          int wave, int lane, int n, int oh0, int ow0) {
  const int kH = a.kH, kW = a.kW, KK = kH * kW;
  const int mg = kc * 32 + 8 * wave, c_lo = kc * 32 / a.dm;
  const float* wt = buf + 8 * wave * KK;      // wave-uniform addresses: broadcast reads
  const float* xs = buf + a.welems;
  int xo[8];                                  // wave-uniform: the channel's plane in the window
  bool live[8];
#pragma unroll
  for (int ch = 0; ch < 8; ++ch) {
    live[ch] = mg + ch < a.Cmid;
    xo[ch] = live[ch] ? ((mg + ch) / a.dm - c_lo) * a.plane : 0;
  }
  int xb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = lane + 64 * j;
    xb[j] = (p / TW) * a.sH * a.HW + (p % TW) * a.sW;
  }
  float acc[2][8];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) acc[j][ch] = 0.f;
  for (int r = 0; r < kH; ++r)
    for (int s = 0; s < kW; ++s) {
      const int t = r * a.HW + s, tap = r * kW + s;
#pragma unroll
      for (int ch = 0; ch < 8; ++ch) {
        const float w = wt[ch * KK + tap];
        acc[0][ch] = __builtin_fmaf(xs[xo[ch] + xb[0] + t], w, acc[0][ch]);
        acc[1][ch] = __builtin_fmaf(xs[xo[ch] + xb[1] + t], w, acc[1][ch]);
      }
    }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = lane + 64 * j;
    const int oh = oh0 + p / TW, ow = ow0 + p % TW;
    const bool pv = oh < a.OH && ow < a.OW;
    v4u g, lo;                                  // g = bf16(sum), lo = bf16(sum - g): the GEMM consumes g + lo
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v0 = pv && live[2 * e] ? acc[j][2 * e] : 0.f, v1 = pv && live[2 * e + 1] ? acc[j][2 * e + 1] : 0.f;
      g[e] = pack2bf(v0, v1);
      lo[e] = pack2bf(v0 - lo_bf(g[e]), v1 - hi_bf(g[e]));
    }
    const int slot = p * 32 + ((wave ^ hswz(p)) << 3);
    *(v4u*)(mid + slot) = g;
    *(v4u*)(mid + TM * 32 + slot) = lo;
    if (mid16 != nullptr && pv && mg < a.Cmid8)
      *(v4u*)(mid16 + (((long)n * a.OH + oh) * a.OW + ow) * a.Cmid8 + mg) = g;
  }
}

template <int TW, int NA>
__global__ __launch_bounds__(256, NA == 4 ? 1 : 2) void sepconv_fwd_kernel(Args a) {
  constexpr int TH = TM / TW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* mid = (bf16_t*)smem;                                  // [128][32] bf16 high parts, then the low parts
  float* stg = (float*)(smem + 2 * MID_BYTES);                  // 2 x [welems weights | xelems window] fp32
  const int stride = a.welems + a.xelems;
  const int lane = threadIdx.x & 63, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.z;
  const int th = blockIdx.x / a.tilesW, tw = blockIdx.x - th * a.tilesW;
  const int oh0 = th * TH, ow0 = tw * TW;
  const int ih0 = oh0 * a.sH - a.pH, iw0 = ow0 * a.sW - a.pW;
  const int nch = a.Cmid32 / 32;
  const long img = (long)a.Cin * a.H * a.W;                     // < 2^29 floats (host predicate)
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + n * img), (short)0, (int)(img * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.wd), (short)0, a.Cmid * a.kH * a.kW * 4, 0x00020000);
  bf16_t* m16 = blockIdx.y == 0 ? a.mid16 : nullptr;

  const int cb = blockIdx.y * (64 * NA) + wave * (16 * NA);     // this wave's first output channel
  const bool active = cb < a.Cout;
  const bf16_t* wrow[NA];
  bool rok[NA];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int row = cb + 16 * q + (lane & 15);
    rok[q] = row < a.Cout8;
    wrow[q] = a.wp + (long)(rok[q] ? row : 0) * a.Cmid32 + 8 * lg;
  }
  const v8s zero = {0, 0, 0, 0, 0, 0, 0, 0};
  v4f acc[NA][FM];
#pragma unroll
  for (int q = 0; q < NA; ++q)
#pragma unroll
    for (int i = 0; i < FM; ++i) acc[q][i] = v4f{0.f, 0.f, 0.f, 0.f};
  v8s af[NA];
#pragma unroll
  for (int q = 0; q < NA; ++q) af[q] = rok[q] ? ld8(wrow[q]) : zero;

  stage(a, rx, rw, 0, stg, wave, lane, ih0, iw0);
  if (nch > 1) stage(a, rx, rw, 1, stg + stride, wave, lane, ih0, iw0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  wg_sync();
  depthwise<TW>(a, 0, stg, mid, m16, wave, lane, n, oh0, ow0);
  wg_sync();

  for (int i = 0; i < nch; ++i) {
    // stage buffer i & 1 was read by the depthwise stage of chunk i, before the last barrier
    if (i + 2 < nch) stage(a, rx, rw, i + 2, stg + (i & 1) * stride, wave, lane, ih0, iw0);
    v8s an[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) an[q] = (rok[q] && i + 1 < nch) ? ld8(wrow[q] + (i + 1) * 32) : zero;
    if (active) {
#pragma unroll
      for (int part = 0; part < 2; ++part) {                     // low parts first or last: the sum is the same to fp32
        const bf16_t* mt = mid + part * (TM * 32);
        v8s b[FM];
#pragma unroll
        for (int f = 0; f < FM; ++f) {
          const int r = 16 * f + (lane & 15);
          b[f] = *(const v8s*)(mt + r * 32 + ((lg ^ hswz(r)) << 3));
        }
#pragma unroll
        for (int f = 0; f < FM; ++f)
#pragma unroll
          for (int q = 0; q < NA; ++q)
            acc[q][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[q], b[f], acc[q][f], 0, 0, 0);
      }
    }
    wg_sync();                                                   // the mid tile has been read by every wave
    if (i + 1 < nch) depthwise<TW>(a, i + 1, stg + ((i + 1) & 1) * stride, mid, m16, wave, lane, n, oh0, ow0);
#pragma unroll
    for (int q = 0; q < NA; ++q) af[q] = an[q];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // chunk i + 2 has landed before anyone reads it
    wg_sync();
  }
  if (!active) return;

  const long plane_o = (long)a.OH * a.OW;
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int k0 = cb + 16 * q + 4 * lg;
#pragma unroll
    for (int f = 0; f < FM; ++f) {
      const int p = 16 * f + (lane & 15);
      const int oh = oh0 + p / TW, ow = ow0 + p % TW;
      if (oh >= a.OH || ow >= a.OW) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + e;
        if (k < a.Cout)
          a.y[((long)n * a.Cout + k) * plane_o + (long)oh * a.OW + ow] = acc[q][f][e] + (a.bias ? a.bias[k] : 0.f);
      }
    }
  }
}

// What the device grants one workgroup (as in convlstm3d.hip): the opt-in limit where the runtime reports one, else
// the plain limit, never more than the 160 KiB this file was written for.
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

int tile_w(const SepConvGeo& g) { return g.OW <= 8 ? 8 : 16; }

// Geometry -> kernel arguments (pointers left null); false when the kernel does not take it.
bool plan(const SepConvGeo& g, Args& a, size_t& lds) {
  if (g.N < 1 || g.N > 65535 || g.Cin < 1 || g.dm < 1 || g.Cout < 1 || g.H < 1 || g.W < 1 || g.OH < 1 || g.OW < 1)
    return false;
  if (g.kH < 1 || g.kH > 7 || g.kW < 1 || g.kW > 7 || g.sH < 1 || g.sH > 2 || g.sW < 1 || g.sW > 2) return false;
  if (g.pH < 0 || g.pH >= g.kH || g.pW < 0 || g.pW >= g.kW) return false;
  if (g.H + 2 * g.pH < g.kH || g.W + 2 * g.pW < g.kW) return false;
  if (g.OH != (g.H + 2 * g.pH - g.kH) / g.sH + 1 || g.OW != (g.W + 2 * g.pW - g.kW) / g.sW + 1) return false;
  // offsets inside an image are 32-bit byte offsets of a buffer resource; everything else is formed in 64 bits
  const long lim = 1l << 29;
  if ((long)g.Cin * g.H >= lim || (long)g.Cin * g.H * g.W >= lim) return false;
  if ((long)g.Cin * g.dm >= (1l << 22) || g.Cout >= (1 << 24) || (long)g.OH * g.OW >= (1l << 31)) return false;
  const int TW = tile_w(g), TH = TM / TW;
  a = Args{};
  a.N = g.N; a.Cin = g.Cin; a.dm = g.dm; a.H = g.H; a.W = g.W; a.Cout = g.Cout; a.OH = g.OH; a.OW = g.OW;
  a.kH = g.kH; a.kW = g.kW; a.sH = g.sH; a.sW = g.sW; a.pH = g.pH; a.pW = g.pW;
  a.Cmid = g.Cin * g.dm; a.Cmid8 = (a.Cmid + 7) / 8 * 8; a.Cmid32 = (a.Cmid + 31) / 32 * 32;
  a.Cout8 = (g.Cout + 7) / 8 * 8;
  a.HH = (TH - 1) * g.sH + g.kH; a.HW = (TW - 1) * g.sW + g.kW; a.plane = a.HH * a.HW;
  int nci = 31 / g.dm + 2;                    // input channels one chunk of 32 mid channels can touch
  if (nci > 32) nci = 32;
  if (nci > g.Cin) nci = g.Cin;
  a.xelems = (nci * a.plane + 255) / 256 * 256;
  a.welems = (32 * g.kH * g.kW + 255) / 256 * 256;
  a.mplane = (unsigned)((1ull << 32) / (unsigned)a.plane) + 1u;
  a.mrow = (unsigned)((1ull << 32) / (unsigned)a.HW) + 1u;
  a.tilesW = (g.OW + TW - 1) / TW;
  if ((long)a.tilesW * ((g.OH + TH - 1) / TH) >= (1l << 31)) return false;
  lds = 2 * (size_t)MID_BYTES + 2 * (size_t)(a.welems + a.xelems) * 4;
  return lds <= lds_cap();
}

template <int TW, int NA>
int launch(const Args& a, size_t lds, hipStream_t st) {
  auto kernel = sepconv_fwd_kernel<TW, NA>;
  if (lds > LDS_DEFAULT &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_cap()) != hipSuccess) {
    (void)hipGetLastError();                  // a runtime that refuses keeps the launch from happening
    return -1;
  }
  const int TH = TM / TW;
  const dim3 grid((unsigned)(a.tilesW * ((a.OH + TH - 1) / TH)), (unsigned)((a.Cout + 64 * NA - 1) / (64 * NA)),
                  (unsigned)a.N);
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a);
  HIP_LAUNCH_CHECK();
  return 0;
}

template <int TW>
int launch_tw(const Args& a, size_t lds, hipStream_t st) {
  // Channel fragments per wave: the fewest Cout blocks (each block repeats the depthwise stage), unless 256-channel
  // blocks would leave fewer than two workgroups per CU (256 CUs) where 128-channel blocks would not.
  const int TH = TM / TW;
  const long tiles = (long)a.tilesW * ((a.OH + TH - 1) / TH) * a.N;
  if (a.Cout <= 64) return launch<TW, 1>(a, lds, st);
  if (a.Cout <= 128 || tiles * ((a.Cout + 255) / 256) < 512) return launch<TW, 2>(a, lds, st);
  return launch<TW, 4>(a, lds, st);
}

}  // namespace

int bigdl_sepconv_supported(const SepConvGeo* g) {
  Args a;
  size_t lds;
  return plan(*g, a, lds) ? 1 : 0;
}

int bigdl_sepconv_fwd(const float* x, const float* wd, const uint16_t* wp, const float* bias, float* y,
                      uint16_t* mid16, const SepConvGeo* g, hipStream_t st) {
  Args a;
  size_t lds;
  if (!plan(*g, a, lds) || !x || !wd || !wp || !y) return -1;
  a.x = x; a.wd = wd; a.wp = wp; a.bias = bias; a.y = y; a.mid16 = mid16;
  return tile_w(*g) == 8 ? launch_tw<8>(a, lds, st) : launch_tw<16>(a, lds, st);
}
