// Fused LSTM time-step kernels for gfx950: one launch per step does the recurrent GEMM on the bf16 MFMA
// and the whole cell (forward) / cell backward + next recurrent-gradient GEMM (backward). One forward and one
// backward kernel serve nn.LSTM, nn.LSTMPeephole and Recurrent(maskZero=True): the GENERAL instantiation takes
// optional peephole terms, an optional per-row mask and a caller-given gate layout; the plain one compiles all of
// that away and is what the unmasked nn.LSTM runs.
//
// Reference: S/nn/LSTM.scala:77-185 (gates i, g, f, o; c' = f*c + i*g; h' = o*tanh(c')), recurrent loop
// S/nn/Recurrent.scala:283-305, fused whole-sequence MKL-DNN RNN S/nn/mkldnn/RNN.scala:36-501;
// S/nn/LSTMPeephole.scala (gate blocks i, f, g, o; peepholes p_i, p_f on c_{t-1} and p_o on c_t),
// S/nn/Recurrent.scala:273-290, 353, 413, 471 (maskZero: a zero input row keeps its state, emits 0 and passes its
// recurrent gradient through unchanged).
//
// Why one launch per step and not a persistent kernel: every step is an all-to-all seam (each workgroup needs
// the whole h_{t-1}); on MI355X a grid barrier costs ~4-5 us at 256 workgroups vs ~1.5 us for a kernel
// boundary (MI355X_MICROARCH price list: barrier-xcd vs boundary), and the HIP-graph-captured step loop has no
// host overhead. What the fusion removes is everything else: the gate pre-activations never touch HBM, the
// cell math runs in the GEMM epilogue, and the weight slice each workgroup reads is the same every step, so
// it stays hot in that XCD's L2.
//
// Both steps are bound by reading the previous step's bf16 state (h_{t-1} or dg_{t+1}) written on all XCDs,
// so tiles are sized to cut that cross-XCD traffic (measured with tools/lstm_micro.py):
// Forward step, workgroup = 16 hidden units x 16*NB batch rows: MFMA 16x16x32 bf16, A = gate rows of W ordered
//   row = unit*4 + gate block, B = h_{t-1}^T; the 4 gates of a (unit, batch) pair meet in LDS, the cell math runs
//   coalesced along the hidden dimension, c stays fp32.
// Backward step, workgroup = 16*NB batch rows x 16*NU hidden units: dh_t = dout_t + dg_{t+1} . W as
//   D[batch][unit] = A(dg16 rows) x B(W^T rows), then the cell backward of each (batch, unit) pair emits
//   dg_t (fp32 for the weight-gradient GEMM, bf16 as the next step's A operand) and dc_{t-1} (in place).
//
// Gate layout: gp.i, gp.f, gp.g, gp.o are the positions of the i, f, g, o blocks inside the [4H] gate axis of xg,
// W16, acts and dg; the GEMM is layout-blind (block q of W16 makes block q of the pre-activations), only the cell
// reads them. The plain instantiation fixes nn.LSTM's (i, g, f, o) at compile time.
//
// Mask (1 = valid row). Forward, masked row: c_t = c_{t-1}, h16[t+1] = h16[t], out = 0, the fp32 h state (a [B, H]
// buffer updated in place by the element's own thread) is left as it is. Backward, masked row: dg_t = 0, dc passes
// through, and the recurrent gradient that arrived for h_t moves on to h_{t-1} through the fp32 carry buffer
// (carry += dg_{t+1} . U); a valid row adds the carry into dh and clears it.
#include "common.h"
#include "kernels.h"
#include "rnn_step.h"

namespace {

struct GatePos { int i, f, g, o; };

// Forward step, fragment-shared: workgroup = 16 hidden units (64 gate rows) x 16*NB batch rows. 64 * max(KS, 4 * NB)
// threads: waves kc < KS own K chunk kc of kl = H / KS, threads < 256 * NB own one (batch, unit) cell each. Per
// k-step a wave loads the 4 W fragments (row tiles mt = 0..3) and the NB h fragments once and issues 4*NB MFMAs, so no
// fragment is loaded twice inside the workgroup: per step the grid moves (H/16) * (B/16/NB) * (64 + 16 NB) rows of K
// (the per-step time tracks those bytes: tools/lstm_micro.py, ~0.12 us per MB at H = 1024). The 64 gate rows a
// workgroup reads are the same every step (L2-resident on its XCD). Gates are summed over the K chunks in LDS, then
// the cell update and all its loads / stores run coalesced along the hidden dimension. Batch rows past B read row 0
// and never store.
template <int NB, int KSMAX, bool GENERAL>
__global__ void __launch_bounds__(1024) lstm_fwd_step_kernel(
    const bf16_t* __restrict__ W16, const bf16_t* __restrict__ h16_prev, const float* __restrict__ xg, long ldx,
    const float* __restrict__ c_prev, float* __restrict__ c_out, float* __restrict__ h_state,
    float* __restrict__ h_out, long ldh, bf16_t* __restrict__ h16_out, float* __restrict__ acts, long lda,
    const float* __restrict__ pI, const float* __restrict__ pF, const float* __restrict__ pO,
    const unsigned char* __restrict__ mask, GatePos gpa, int B, int H, int KS) {
  __shared__ float gl[KSMAX][16 * NB][16][5];                // [K chunk][batch][unit][gate block] (+1 pad)
  const GatePos gp = GENERAL ? gpa : GatePos{0, 2, 1, 3};
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
    xi = x[(long)gp.i * H]; xc = x[(long)gp.g * H]; xf = x[(long)gp.f * H]; xo = x[(long)gp.o * H];
    cp = c_prev != nullptr ? c_prev[(long)bs * H + j] : 0.f;
    if constexpr (GENERAL) {
      if (pI != nullptr) { wi = pI[j]; wf = pF[j]; wo = pO[j]; }
      if (mask != nullptr) {
        valid = mask[bs] != 0;
        hp16 = h16_prev != nullptr ? h16_prev[(long)bs * H + j] : (bf16_t)0;
      }
    }
  }
  if (h16_prev != nullptr && kc < KS) {
    v4f acc[4][NB];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[mt][t] = v4f{0.f, 0.f, 0.f, 0.f};
    const int kl = H / KS;
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
    // mfma_tiles<4, NB, true> written out with the loads of a k-step grouped by k-step, not by operand: the shared
    // form compiles to a longer kernel here and measured 0.1 us slower per step at B = 64 (tools/lstm_micro.py)
    constexpr int G = 4;
    const int steps = kl / 32;
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
  if constexpr (GENERAL) {
    if (!valid) {                    // masked row: the state carries, the output is 0
      c_out[bj] = cp;
      h_out[(long)b * ldh + j] = 0.f;
      h16_out[bj] = hp16;
      a[0] = 0.f; a[H] = 0.f; a[2 * H] = 0.f; a[3 * H] = 0.f;
      return;
    }
  }
  float gi = 0.f, gf = 0.f, gc = 0.f, go = 0.f;
  if (h16_prev != nullptr)
    for (int k = 0; k < KS; ++k) {   // the gate blocks are picked by LDS address (compile-time offsets when plain)
      const float* q = gl[k][tile * 16 + m][n];
      gi += q[gp.i]; gf += q[gp.f]; gc += q[gp.g]; go += q[gp.o];
    }
  float ai = gi + xi, af = gf + xf, ao = go + xo;
  if constexpr (GENERAL) { ai += wi * cp; af += wf * cp; }
  const float ig = sigm(ai), fg = sigm(af), gg = tanh_f(gc + xc);
  const float c = fg * cp + ig * gg;
  if constexpr (GENERAL) ao += wo * c;
  const float og = sigm(ao);
  const float h = og * tanh_f(c);
  c_out[bj] = c;
  if constexpr (GENERAL) {
    if (h_state != nullptr) h_state[bj] = h;
  }
  h_out[(long)b * ldh + j] = h;
  h16_out[bj] = f2bf(h);
  a[(long)gp.i * H] = ig; a[(long)gp.g * H] = gg; a[(long)gp.f * H] = fg; a[(long)gp.o * H] = og;
}

// Backward step. Workgroup = 16*NB batch rows x 16*NU hidden units, exactly KS waves splitting K = 4H: rec =
// dg_{t+1} . W as D[batch][unit] = A(dg16 rows) x B(W^T rows), partials summed in LDS; dh_t = dout_t + dh_ext + rec
// (+ carry), then the cell backward of each (batch, unit) pair emits dg_t (fp32 for the weight gradients, bf16 as the
// next step's A operand) and dc_{t-1} (in place). dc and carry are read and written by the element's own thread only.
template <int NB, int NU, bool GENERAL>
__global__ void __launch_bounds__(1024) lstm_bwd_step_kernel(
    const bf16_t* __restrict__ WT16, const bf16_t* __restrict__ dg16_next, const float* __restrict__ dout, long ldd,
    const float* __restrict__ dh_ext, const float* __restrict__ acts, long lda, const float* __restrict__ c_prev,
    const float* __restrict__ c_t, float* __restrict__ dc, float* __restrict__ carry, float* __restrict__ dg_out,
    long ldg, bf16_t* __restrict__ dg16_out, const float* __restrict__ pI, const float* __restrict__ pF,
    const float* __restrict__ pO, const unsigned char* __restrict__ mask, GatePos gpa, int B, int H, int KS) {
  __shared__ float red[NU * NB][16][16][17];                 // [unit tile x batch tile][K chunk][batch][unit]
  const GatePos gp = GENERAL ? gpa : GatePos{0, 2, 1, 3};
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
    ig = a[(long)gp.i * H]; gg = a[(long)gp.g * H]; fg = a[(long)gp.f * H]; og = a[(long)gp.o * H];
    c = c_t[bj];
    cp = c_prev != nullptr ? c_prev[bj] : 0.f;
    dcn = dc[bj];
    if constexpr (GENERAL) {
      if (carry != nullptr) cin = carry[bj];
      if (pI != nullptr) { wi = pI[j]; wf = pF[j]; wo = pO[j]; }
      if (mask != nullptr) valid = mask[bs] != 0;
    }
  }
  v4f acc[NU][NB];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int t = 0; t < NB; ++t) acc[u][t] = v4f{0.f, 0.f, 0.f, 0.f};
  if (dg16_next != nullptr) {
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
    mfma_tiles<NU, NB, false>(pw, pv, kl, acc);
  }
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[u * NB + t][wave][kh * 4 + i][r] = acc[u][t][i];  // D[row = batch][col = unit]
  __syncthreads();
  if (!live) return;
  float* g = dg_out + (long)b * ldg + j;
  bf16_t* g16 = dg16_out + (long)b * 4 * H + j;
  // dout + dh_ext, then the K chunks in order (a masked row sums them alone: they are what it hands on), then the carry
  if (!valid) dh = 0.f;
  for (int k = 0; k < KS; ++k) dh += red[tu * NB + tb][k][m][n];
  if constexpr (GENERAL) {
    if (!valid) {                    // masked row: no gate gradient, dc untouched, the recurrent gradient moves on
      if (carry != nullptr) carry[bj] = cin + dh;
      g[0] = 0.f; g[H] = 0.f; g[2 * H] = 0.f; g[3 * H] = 0.f;
      g16[0] = 0; g16[H] = 0; g16[2 * H] = 0; g16[3 * H] = 0;
      return;
    }
    dh += cin;
    if (carry != nullptr) carry[bj] = 0.f;
  }
  const float tc = tanh_f(c);
  const float dog = dh * tc * og * (1.f - og);
  float dcv = dh * og * (1.f - tc * tc) + dcn;
  if constexpr (GENERAL) dcv += dog * wo;
  const float di = dcv * gg * ig * (1.f - ig);
  const float df = dcv * cp * fg * (1.f - fg);
  const float dgg = dcv * ig * (1.f - gg * gg);
  float dcp = dcv * fg;
  if constexpr (GENERAL) dcp += di * wi + df * wf;
  dc[bj] = dcp;                                          // flows into c_{t-1}; same thread reads and writes
  g[(long)gp.i * H] = di; g[(long)gp.g * H] = dgg; g[(long)gp.f * H] = df; g[(long)gp.o * H] = dog;
  g16[(long)gp.i * H] = f2bf(di); g16[(long)gp.g * H] = f2bf(dgg);
  g16[(long)gp.f * H] = f2bf(df); g16[(long)gp.o * H] = f2bf(dog);
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

// Batch tiles per workgroup: 2 once the 1-tile grid exceeds one workgroup per CU (a second dispatch round costs a
// whole extra step latency, and the pair shares every weight fragment); BIGDL_LSTM_NB forces 1 or 2.
int lstm_nb(int H, int B) {
  static const int env = [] { const char* e = getenv("BIGDL_LSTM_NB"); return e ? atoi(e) : 0; }();
  if (env == 1 || env == 2) return env;
  return (long)(H / 16) * ((B + 15) / 16) > 256 ? 2 : 1;
}

// Forward tile rule: K chunks of >= 32 over at most 16 (NB = 1) / 8 (NB = 2) waves; one batch tile where the K
// chunks give fewer than the 256 cell threads per tile that two would need; the workgroup is padded to those cell
// threads where H has too few K chunks (the padding waves skip the GEMM), so every H % 32 == 0 runs.
struct FwdTile { int NB, KS, waves; };
FwdTile lstm_fwd_tile(int H, int B) {
  int NB = lstm_nb(H, B);
  int KS = 1;
  for (int k = NB == 2 ? 8 : 16; k > 1; --k)
    if (H % (k * 32) == 0) { KS = k; break; }
  if (64 * KS < 256 * NB) NB = 1;
  return {NB, KS, KS > 4 * NB ? KS : 4 * NB};
}

// Backward tile rule: K = 4H over at most 16 waves, at least 4 so all 256 cell threads exist (4H / 4 = H is a
// multiple of 32 too); 2 batch tiles need 512 cell threads. 32 hidden units per workgroup too once the 2-batch-tile
// grid still exceeds one workgroup per CU (B = 256, H = 1024: 27.7 -> 19.6 us per step; at 256 workgroups or fewer
// the halved grid loses, B = 128: 15.4 -> 19.0 us); needs 1024 cell threads (KS = 16). BIGDL_LSTM_NU forces 1 or 2.
struct BwdTile { int NB, NU, KS; };
BwdTile lstm_bwd_tile(int H, int B) {
  static const int nu_env = [] { const char* e = getenv("BIGDL_LSTM_NU"); return e ? atoi(e) : 0; }();
  const int ks0 = ksplit(4 * H, 16);
  const int KS = ks0 < 4 ? 4 : ks0;
  const int NB = KS * 64 < 512 ? 1 : lstm_nb(H, B);
  const bool nu_ok = NB == 2 && KS == 16;
  const int NU = !nu_ok ? 1 : (nu_env == 1 || nu_env == 2) ? nu_env
                                                             : ((long)(H / 16) * ((B + 31) / 32) > 256 ? 2 : 1);
  return {NB, NU, KS};
}

}  // namespace

int bigdl_lstm_fwd_step(const uint16_t* W16, const uint16_t* h16_prev, const float* xg, long ldx, const float* c_prev,
                        float* c_out, float* h_state, float* h_out, long ldh, uint16_t* h16_out, float* acts, long lda,
                        const float* pI, const float* pF, const float* pO, const unsigned char* mask, int gi, int gf,
                        int gg, int go, int B, int H, hipStream_t st) {
  if (H % 32 != 0 || H <= 0 || B <= 0 || !gate_perm(gi, gf, gg, go)) return -1;
  if ((pI != nullptr) != (pF != nullptr) || (pI != nullptr) != (pO != nullptr)) return -1;
  // the plain instantiation: nn.LSTM's layout and nothing optional
  const bool general =
      pI != nullptr || mask != nullptr || h_state != nullptr || gi != 0 || gf != 2 || gg != 1 || go != 3;
  const FwdTile t = lstm_fwd_tile(H, B);
  const auto kernel = t.NB == 2 ? (general ? lstm_fwd_step_kernel<2, 8, true> : lstm_fwd_step_kernel<2, 8, false>)
                                : (general ? lstm_fwd_step_kernel<1, 16, true> : lstm_fwd_step_kernel<1, 16, false>);
  dim3 grid(H / 16, (B + 16 * t.NB - 1) / (16 * t.NB));
  kernel<<<grid, 64 * t.waves, 0, st>>>(W16, h16_prev, xg, ldx, c_prev, c_out, h_state, h_out, ldh, h16_out, acts, lda,
                                        pI, pF, pO, mask, GatePos{gi, gf, gg, go}, B, H, t.KS);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_lstm_bwd_step(const uint16_t* WT16, const uint16_t* dg16_next, const float* dout, long ldd,
                        const float* dh_ext, const float* acts, long lda, const float* c_prev, const float* c_t,
                        float* dc, float* carry, float* dg_out, long ldg, uint16_t* dg16_out, const float* pI,
                        const float* pF, const float* pO, const unsigned char* mask, int gi, int gf, int gg, int go,
                        int B, int H, hipStream_t st) {
  if (H % 32 != 0 || H <= 0 || B <= 0 || !gate_perm(gi, gf, gg, go)) return -1;
  if ((pI != nullptr) != (pF != nullptr) || (pI != nullptr) != (pO != nullptr)) return -1;
  if (mask != nullptr && carry == nullptr) return -1;
  const bool general = pI != nullptr || mask != nullptr || carry != nullptr || gi != 0 || gf != 2 || gg != 1 || go != 3;
  const BwdTile t = lstm_bwd_tile(H, B);
  const auto kernel = t.NU == 2   ? (general ? lstm_bwd_step_kernel<2, 2, true> : lstm_bwd_step_kernel<2, 2, false>)
                      : t.NB == 2 ? (general ? lstm_bwd_step_kernel<2, 1, true> : lstm_bwd_step_kernel<2, 1, false>)
                                  : (general ? lstm_bwd_step_kernel<1, 1, true> : lstm_bwd_step_kernel<1, 1, false>);
  dim3 grid(H / (16 * t.NU), (B + 16 * t.NB - 1) / (16 * t.NB));
  kernel<<<grid, 64 * t.KS, 0, st>>>(WT16, dg16_next, dout, ldd, dh_ext, acts, lda, c_prev, c_t, dc, carry, dg_out, ldg,
                                     dg16_out, pI, pF, pO, mask, GatePos{gi, gf, gg, go}, B, H, t.KS);
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
