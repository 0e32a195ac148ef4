// Fused LSTM time-step kernels with a general cell epilogue for gfx950: optional peephole terms (nn.LSTMPeephole),
// an optional per-row mask (Recurrent(maskZero=True)) and a caller-given gate layout. One launch per step does the
// recurrent GEMM on the bf16 MFMA and the whole cell (forward) / cell backward + next recurrent-gradient GEMM
// (backward), like csrc/lstm.hip, which stays the specialised path of the unmasked nn.LSTM.
//
// Reference: S/nn/LSTMPeephole.scala (gate blocks i, f, g, o; peepholes p_i, p_f on c_{t-1} and p_o on c_t),
// S/nn/Recurrent.scala:273-290, 353, 413, 471 (maskZero: a zero input row keeps its state, emits 0 and passes its
// recurrent gradient through unchanged), S/nn/LSTM.scala:77-185 (gate blocks i, g, f, o).
//
// Gate layout: gi, gf, gg, go are the positions of the i, f, g, o blocks inside the [4H] gate axis of xg, W16, acts
// and dg; the GEMM is layout-blind (block q of W16 makes block q of the pre-activations), only the cell reads them.
//
// Forward step = the fragment-shared form of csrc/lstm.hip (workgroup = 16 hidden units x 16*NB batch rows, wave kc
// owns K chunk kc, every W / h fragment loaded once per workgroup), with the workgroup sized by the cell phase where
// H has too few K chunks, so every H % 32 == 0 runs it. Backward step = 16*NB batch rows x 16*NU hidden units, waves
// splitting K = 4H.
//
// Mask (1 = valid row). Forward, masked row: c_t = c_{t-1}, h16[t+1] = h16[t], out = 0, the fp32 h state (a [B, H]
// buffer updated in place by the element's own thread) is left as it is. Backward, masked row: dg_t = 0, dc passes
// through, and the recurrent gradient that arrived for h_t moves on to h_{t-1} through the fp32 carry buffer
// (carry += dg_{t+1} . U); a valid row adds the carry into dh and clears it.
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  const float e = __expf(-2.f * fabsf(x));
  const float t = (1.f - e) / (1.f + e);
  return x < 0.f ? -t : t;
}

__device__ __forceinline__ v8s ld8(const bf16_t* p) { return *(const v8s*)p; }

struct GatePos { int i, f, g, o; };

// Forward step. 64 * max(KS, 4 * NB) threads: waves kc < KS own K chunk kc of kl = H / KS, threads < 256 * NB own one
// (batch, unit) cell each. Batch rows past B read row 0 and never store.
template <int NB, int KSMAX>
__global__ void __launch_bounds__(1024) lstm_peep_fwd_step_kernel(
    const bf16_t* __restrict__ W16, const bf16_t* __restrict__ h16_prev, const float* __restrict__ xg, long ldx,
    const float* __restrict__ c_prev, float* __restrict__ c_out, float* __restrict__ h_state,
    float* __restrict__ h_out, long ldh, bf16_t* __restrict__ h16_out, float* __restrict__ acts, long lda,
    const float* __restrict__ pI, const float* __restrict__ pF, const float* __restrict__ pO,
    const unsigned char* __restrict__ mask, GatePos gp, int B, int H, int KS) {
  __shared__ float gl[KSMAX][16 * NB][16][5];                // [K chunk][batch][unit][gate block] (+1 pad)
  const int lane = threadIdx.x & 63, kc = threadIdx.x >> 6;
  const int r = lane & 15, kh = lane >> 4;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16 * NB;
  const bool cell = threadIdx.x < 256 * NB;
  const int tile = threadIdx.x >> 8;
  const int m = (threadIdx.x >> 4) & 15, n = threadIdx.x & 15;
  const int b = b0 + tile * 16 + m, j = j0 + n;
  const bool live = cell && b < B;
  const int bs = b < B ? b : 0;
  float xi = 0.f, xf = 0.f, xc = 0.f, xo = 0.f, cp = 0.f, wi = 0.f, wf = 0.f, wo = 0.f;
  bool valid = true;
  bf16_t hp16 = 0;
  if (cell) {                        // cell operands in flight while the GEMM runs
    const float* x = xg + (long)bs * ldx + j;
    xi = x[(long)gp.i * H]; xf = x[(long)gp.f * H]; xc = x[(long)gp.g * H]; xo = x[(long)gp.o * H];
    cp = c_prev != nullptr ? c_prev[(long)bs * H + j] : 0.f;
    if (pI != nullptr) { wi = pI[j]; wf = pF[j]; wo = pO[j]; }
    if (mask != nullptr) {
      valid = mask[bs] != 0;
      hp16 = h16_prev != nullptr ? h16_prev[(long)bs * H + j] : (bf16_t)0;
    }
  }
  if (h16_prev != nullptr && kc < KS) {
    v4f acc[4][NB];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[mt][t] = v4f{0.f, 0.f, 0.f, 0.f};
    const int kl = H / KS, steps = kl / 32;
    const bf16_t* pw[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)                                   // A row r = unit*4 + gate block
      pw[mt] = W16 + (long)((r & 3) * H + j0 + mt * 4 + (r >> 2)) * H + kc * kl + kh * 8;
    const bf16_t* pv[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int bl = b0 + t * 16 + r;        // batch rows past B read row 0: their columns are never stored
      pv[t] = h16_prev + (long)(bl < B ? bl : 0) * H + kc * kl + kh * 8;
    }
    constexpr int G = 4;
    int s = 0;
    for (; s + G <= steps; s += G) {
      v8s a[G][4], v[NB][G];
#pragma unroll
      for (int i = 0; i < G; ++i) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a[i][mt] = ld8(pw[mt] + (s + i) * 32);
#pragma unroll
        for (int t = 0; t < NB; ++t) v[t][i] = ld8(pv[t] + (s + i) * 32);
      }
#pragma unroll
      for (int i = 0; i < G; ++i)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int t = 0; t < NB; ++t)
            acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][mt], v[t][i], acc[mt][t], 0, 0, 0);
    }
    for (; s < steps; ++s) {
      v8s a[4], v[NB];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) a[mt] = ld8(pw[mt] + s * 32);
#pragma unroll
      for (int t = 0; t < NB; ++t) v[t] = ld8(pv[t] + s * 32);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int t = 0; t < NB; ++t)
          acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], v[t], acc[mt][t], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) gl[kc][t * 16 + r][mt * 4 + kh][i] = acc[mt][t][i];   // D[unit*4+block][batch]
  }
  __syncthreads();
  if (!live) return;
  const long bj = (long)b * H + j;
  float* a = acts + (long)b * lda + j;
  if (!valid) {                      // masked row: the state carries, the output is 0
    c_out[bj] = cp;
    h_out[(long)b * ldh + j] = 0.f;
    h16_out[bj] = hp16;
    a[0] = 0.f; a[H] = 0.f; a[2 * H] = 0.f; a[3 * H] = 0.f;
    return;
  }
  float gi = 0.f, gf = 0.f, gc = 0.f, go = 0.f;
  if (h16_prev != nullptr)
    for (int k = 0; k < KS; ++k) {   // the gate blocks are picked by LDS address, not by register index
      const float* q = gl[k][tile * 16 + m][n];
      gi += q[gp.i]; gf += q[gp.f]; gc += q[gp.g]; go += q[gp.o];
    }
  const float ig = sigm(gi + xi + wi * cp), fg = sigm(gf + xf + wf * cp), gg = tanh_f(gc + xc);
  const float c = fg * cp + ig * gg;
  const float og = sigm(go + xo + wo * c);
  const float h = og * tanh_f(c);
  c_out[bj] = c;
  if (h_state != nullptr) h_state[bj] = h;
  h_out[(long)b * ldh + j] = h;
  h16_out[bj] = f2bf(h);
  a[(long)gp.i * H] = ig; a[(long)gp.f * H] = fg; a[(long)gp.g * H] = gg; a[(long)gp.o * H] = og;
}

// NS x NV output tiles of the backward GEMM: acc[u][t] += V[t] x S[u] over K, fragments of a group of k-steps all
// loaded before the group's MFMAs (one memory round trip per group).
template <int NS, int NV>
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
          acc[u][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n][i], a[u][i], acc[u][n], 0, 0, 0);
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
        acc[u][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n], a[u], acc[u][n], 0, 0, 0);
  }
}

// Backward step. Workgroup = 16*NB batch rows x 16*NU hidden units, KS waves splitting K = 4H: rec = dg_{t+1} . W as
// D[batch][unit] = A(dg16 rows) x B(W^T rows), partials summed in LDS; dh_t = dout_t + dh_ext + rec + carry, then
// the cell backward of each (batch, unit) pair emits dg_t (fp32 for the weight gradients, bf16 as the next step's A
// operand) and dc_{t-1} (in place). dc and carry are read and written by the element's own thread only.
template <int NB, int NU>
__global__ void __launch_bounds__(1024) lstm_peep_bwd_step_kernel(
    const bf16_t* __restrict__ WT16, const bf16_t* __restrict__ dg16_next, const float* __restrict__ dout, long ldd,
    const float* __restrict__ dh_ext, const float* __restrict__ acts, long lda, const float* __restrict__ c_prev,
    const float* __restrict__ c_t, float* __restrict__ dc, float* __restrict__ carry, float* __restrict__ dg_out,
    long ldg, bf16_t* __restrict__ dg16_out, const float* __restrict__ pI, const float* __restrict__ pF,
    const float* __restrict__ pO, const unsigned char* __restrict__ mask, GatePos gp, int B, int H, int KS) {
  __shared__ float red[NU * NB][16][16][17];                 // [unit tile x batch tile][K chunk][batch][unit]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kh = lane >> 4;
  const int j0 = blockIdx.x * 16 * NU, b0 = blockIdx.y * 16 * NB;
  const bool cell = threadIdx.x < 256 * NB * NU;
  const int tile = threadIdx.x >> 8, tb = tile % NB, tu = tile / NB;
  const int m = (threadIdx.x >> 4) & 15, n = threadIdx.x & 15;
  const int b = b0 + tb * 16 + m, j = j0 + tu * 16 + n;
  const bool live = cell && b < B;
  const int bs = b < B ? b : 0;
  const long bj = (long)bs * H + j;
  float dh = 0.f, ig = 0.f, gg = 0.f, fg = 0.f, og = 0.f, c = 0.f, cp = 0.f, dcn = 0.f, cin = 0.f;
  float wi = 0.f, wf = 0.f, wo = 0.f;
  bool valid = true;
  if (cell) {                        // cell operands in flight while the GEMM runs
    if (dout != nullptr) dh += dout[(long)bs * ldd + j];
    if (dh_ext != nullptr) dh += dh_ext[bj];
    const float* a = acts + (long)bs * lda + j;
    ig = a[(long)gp.i * H]; fg = a[(long)gp.f * H]; gg = a[(long)gp.g * H]; og = a[(long)gp.o * H];
    c = c_t[bj];
    cp = c_prev != nullptr ? c_prev[bj] : 0.f;
    dcn = dc[bj];
    if (carry != nullptr) cin = carry[bj];
    if (pI != nullptr) { wi = pI[j]; wf = pF[j]; wo = pO[j]; }
    if (mask != nullptr) valid = mask[bs] != 0;
  }
  if (dg16_next != nullptr && wave < KS) {
    v4f acc[NU][NB];
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[u][t] = v4f{0.f, 0.f, 0.f, 0.f};
    const long G = 4L * H;
    const int kl = (int)(G / KS);
    // batch rows past B read row 0: an A row only feeds its own output row, whose thread never stores
    const bf16_t* pv[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int ba = b0 + t * 16 + r;
      pv[t] = dg16_next + (long)(ba < B ? ba : 0) * G + (long)wave * kl + kh * 8;
    }
    const bf16_t* pw[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) pw[u] = WT16 + (long)(j0 + u * 16 + r) * G + (long)wave * kl + kh * 8;
    mfma_tiles<NU, NB>(pw, pv, kl, acc);
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[u * NB + t][wave][kh * 4 + i][r] = acc[u][t][i];  // D[batch][unit]
  }
  __syncthreads();
  if (!live) return;
  float rec = 0.f;
  if (dg16_next != nullptr)
    for (int k = 0; k < KS; ++k) rec += red[tu * NB + tb][k][m][n];
  float* g = dg_out + (long)b * ldg + j;
  bf16_t* g16 = dg16_out + (long)b * 4 * H + j;
  if (!valid) {                      // masked row: no gate gradient, dc untouched, the recurrent gradient moves on
    if (carry != nullptr) carry[bj] = cin + rec;
    g[0] = 0.f; g[H] = 0.f; g[2 * H] = 0.f; g[3 * H] = 0.f;
    g16[0] = 0; g16[H] = 0; g16[2 * H] = 0; g16[3 * H] = 0;
    return;
  }
  dh += rec + cin;
  if (carry != nullptr) carry[bj] = 0.f;
  const float tc = tanh_f(c);
  const float dog = dh * tc * og * (1.f - og);
  const float dcv = dh * og * (1.f - tc * tc) + dcn + dog * wo;
  const float di = dcv * gg * ig * (1.f - ig);
  const float df = dcv * cp * fg * (1.f - fg);
  const float dgg = dcv * ig * (1.f - gg * gg);
  dc[bj] = dcv * fg + di * wi + df * wf;                 // flows into c_{t-1}; same thread reads and writes
  g[(long)gp.i * H] = di; g[(long)gp.f * H] = df; g[(long)gp.g * H] = dgg; g[(long)gp.o * H] = dog;
  g16[(long)gp.i * H] = f2bf(di); g16[(long)gp.f * H] = f2bf(df);
  g16[(long)gp.g * H] = f2bf(dgg); g16[(long)gp.o * H] = f2bf(dog);
}

// Peephole weight gradients, stage 1: dp_i = sum di_ * c_{t-1}, dp_f = sum df_ * c_{t-1}, dp_o = sum do_ * c_t over
// all rows (t, b). Workgroup = 32 hidden units x 8 row lanes over row slice blockIdx.y of `chunk` rows; each row lane
// sums its rows in ascending order, the 8 lanes are added in lane order: part[slice][3][H]. No atomics.
__global__ void __launch_bounds__(256) lstm_peep_wgrad_part_kernel(
    const float* __restrict__ dg, long dg_sb, long dg_st, const float* __restrict__ cs, const float* __restrict__ c0,
    float* __restrict__ part, GatePos gp, int T, int B, int H, long chunk) {
  __shared__ float red[3][8][33];
  const int n = threadIdx.x & 31, y = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + n;
  const long rows = (long)T * B;
  const long lo = blockIdx.y * chunk, hi = lo + chunk < rows ? lo + chunk : rows;
  float si = 0.f, sf = 0.f, so = 0.f;
  for (long row = lo + y; row < hi; row += 8) {
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    const float* d = dg + b * dg_sb + t * dg_st + j;
    const float ct = cs[row * H + j];
    const float cp = t > 0 ? cs[(row - B) * H + j] : (c0 != nullptr ? c0[(long)b * H + j] : 0.f);
    si += d[(long)gp.i * H] * cp;
    sf += d[(long)gp.f * H] * cp;
    so += d[(long)gp.o * H] * ct;
  }
  red[0][y][n] = si; red[1][y][n] = sf; red[2][y][n] = so;
  __syncthreads();
  if (threadIdx.x < 96) {
    const int k = threadIdx.x >> 5;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += red[k][q][n];
    part[((long)blockIdx.y * 3 + k) * H + j] = v;
  }
}

// Stage 2: out[3][H] = sum over the slices, in slice order.
__global__ void __launch_bounds__(256) lstm_peep_wgrad_sum_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                  int S, int n3h) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3h) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += part[(long)s * n3h + e];
  out[e] = v;
}

bool gate_perm(int gi, int gf, int gg, int go) {
  if ((gi | gf | gg | go) < 0 || gi > 3 || gf > 3 || gg > 3 || go > 3) return false;
  return ((1 << gi) | (1 << gf) | (1 << gg) | (1 << go)) == 15;
}

// K-split factor of the backward GEMM: chunks of >= 256 (8 k-steps), at most `cap` waves per output tile.
int ksplit(int K, int cap) {
  int ks = K / 256;
  if (ks < 1) ks = 1;
  if (ks > cap) ks = cap;
  while (ks > 1 && (K % (ks * 32)) != 0) --ks;
  return ks;
}

}  // namespace

int bigdl_lstm_peep_fwd_step(const uint16_t* W16, const uint16_t* h16_prev, const float* xg, long ldx,
                             const float* c_prev, float* c_out, float* h_state, float* h_out, long ldh,
                             uint16_t* h16_out, float* acts, long lda, const float* pI, const float* pF,
                             const float* pO, const unsigned char* mask, int gi, int gf, int gg, int go, int B, int H,
                             hipStream_t st) {
  if (H % 32 != 0 || H <= 0 || B <= 0 || !gate_perm(gi, gf, gg, go)) return -1;
  if ((pI != nullptr) != (pF != nullptr) || (pI != nullptr) != (pO != nullptr)) return -1;
  // two batch tiles per workgroup once the 1-tile grid exceeds one workgroup per CU (the pair shares every weight
  // fragment); K chunks of >= 32 over at most 16 (NB = 1) / 8 (NB = 2) waves
  const int NB = (long)(H / 16) * ((B + 15) / 16) > 256 ? 2 : 1;
  int KS = 1;
  for (int k = NB == 2 ? 8 : 16; k > 1; --k)
    if (H % (k * 32) == 0) { KS = k; break; }
  const int waves = KS > 4 * NB ? KS : 4 * NB;               // 256 cell threads per batch tile
  const GatePos gp{gi, gf, gg, go};
  dim3 grid(H / 16, (B + 16 * NB - 1) / (16 * NB));
  if (NB == 2)
    lstm_peep_fwd_step_kernel<2, 8><<<grid, 64 * waves, 0, st>>>(W16, h16_prev, xg, ldx, c_prev, c_out, h_state, h_out,
                                                                 ldh, h16_out, acts, lda, pI, pF, pO, mask, gp, B, H,
                                                                 KS);
  else
    lstm_peep_fwd_step_kernel<1, 16><<<grid, 64 * waves, 0, st>>>(W16, h16_prev, xg, ldx, c_prev, c_out, h_state,
                                                                  h_out, ldh, h16_out, acts, lda, pI, pF, pO, mask, gp,
                                                                  B, H, KS);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_lstm_peep_bwd_step(const uint16_t* WT16, const uint16_t* dg16_next, const float* dout, long ldd,
                             const float* dh_ext, const float* acts, long lda, const float* c_prev, const float* c_t,
                             float* dc, float* carry, float* dg_out, long ldg, uint16_t* dg16_out, const float* pI,
                             const float* pF, const float* pO, const unsigned char* mask, int gi, int gf, int gg,
                             int go, int B, int H, hipStream_t st) {
  if (H % 32 != 0 || H <= 0 || B <= 0 || !gate_perm(gi, gf, gg, go)) return -1;
  if ((pI != nullptr) != (pF != nullptr) || (pI != nullptr) != (pO != nullptr)) return -1;
  const int ks0 = ksplit(4 * H, 16);
  const int KS = ks0 < 4 ? 4 : ks0;                          // 4H / 4 = H is a multiple of 32 too
  // tile rules of csrc/lstm.hip's backward step: 2 batch tiles past one workgroup per CU (needs 512 cell threads),
  // 32 hidden units too once that grid still exceeds it (needs 1024)
  const int NB = KS * 64 >= 512 && (long)(H / 16) * ((B + 15) / 16) > 256 ? 2 : 1;
  const int NU = NB == 2 && KS == 16 && (long)(H / 16) * ((B + 31) / 32) > 256 ? 2 : 1;
  const GatePos gp{gi, gf, gg, go};
  dim3 grid(H / (16 * NU), (B + 16 * NB - 1) / (16 * NB));
  if (NU == 2)
    lstm_peep_bwd_step_kernel<2, 2><<<grid, 64 * KS, 0, st>>>(WT16, dg16_next, dout, ldd, dh_ext, acts, lda, c_prev,
                                                              c_t, dc, carry, dg_out, ldg, dg16_out, pI, pF, pO, mask,
                                                              gp, B, H, KS);
  else if (NB == 2)
    lstm_peep_bwd_step_kernel<2, 1><<<grid, 64 * KS, 0, st>>>(WT16, dg16_next, dout, ldd, dh_ext, acts, lda, c_prev,
                                                              c_t, dc, carry, dg_out, ldg, dg16_out, pI, pF, pO, mask,
                                                              gp, B, H, KS);
  else
    lstm_peep_bwd_step_kernel<1, 1><<<grid, 64 * KS, 0, st>>>(WT16, dg16_next, dout, ldd, dh_ext, acts, lda, c_prev,
                                                              c_t, dc, carry, dg_out, ldg, dg16_out, pI, pF, pO, mask,
                                                              gp, B, H, KS);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_lstm_peep_wgrad_slices(long rows) {
  long s = rows / 128;
  return (int)(s < 1 ? 1 : s > 64 ? 64 : s);
}

int bigdl_lstm_peep_wgrad(const float* dg, long dg_sb, long dg_st, const float* cs, const float* c0, float* part,
                          float* out, int gi, int gf, int gg, int go, int T, int B, int H, hipStream_t st) {
  if (H % 32 != 0 || H <= 0 || B <= 0 || T <= 0 || !gate_perm(gi, gf, gg, go)) return -1;
  const long rows = (long)T * B;
  const int S = bigdl_lstm_peep_wgrad_slices(rows);
  const long chunk = (rows + S - 1) / S;
  const GatePos gp{gi, gf, gg, go};
  lstm_peep_wgrad_part_kernel<<<dim3(H / 32, S), 256, 0, st>>>(dg, dg_sb, dg_st, cs, c0, part, gp, T, B, H, chunk);
  HIP_LAUNCH_CHECK();
  lstm_peep_wgrad_sum_kernel<<<(3 * H + 255) / 256, 256, 0, st>>>(part, out, S, 3 * H);
  HIP_LAUNCH_CHECK();
  return 0;
}
