// Fused BinaryTreeLSTM level kernels for gfx950: one launch per tree level and direction over every node of that
// height in the whole batch of trees, the gate GEMM on the bf16 MFMA and the cell in its epilogue.
//
// Reference: S/nn/BinaryTreeLSTM.scala:33-573 (leaf module c = W_c x, h = sigmoid(W_o x) * tanh(c); composer gates
// i, lf, rf, u, o from (h_l, h_r); c = i*u + lf*c_l + rf*c_r; h = o * tanh(c), tanh(c) without the output gate).
//
// Layout: slot-major state, written by the children. The host schedule (bigdl_treelstm_schedule) gives every
// composer node a slot, global over all levels, and every node the slot of its parent and the side it hangs on. A
// node's epilogue stores its bf16 h and fp32 c into its PARENT's slot, hch16 / cch [slot][side * Hp + unit], so
//   - the forward B operand of a composer row is one contiguous K = 2 * Hp row (no gather by child index),
//   - that same buffer is the dense operand of the weight-gradient GEMM after the sweep (dW = dg^T . hch16),
//   - the backward hands dc * lf / dc * rf down the same way (dcp [slot][side * Hp + unit], read by the child).
// A tree node has exactly one parent (the schedule checks it), so every element has one writer: plain stores, no
// atomics, a fixed summation order, bitwise-reproducible results. Slot Z (one past the last composer) is all zeros in
// every slot buffer and is never written: it is the parent of the roots and what the padding rows of a tile read.
//
// Table: 8 ints per row (node row b * N + n or -1 for a padding row, own slot, parent slot, side, input row
// b * L + word for leaves). A level's rows are [children on the left | children on the right], each group padded to
// 16 rows, so a 16-row MFMA tile of the backward reads one of W_left / W_right. Padding rows never store.
//
// Padding of the hidden axis: Hp = H rounded up to 32, the packed weights and biases are zero there. A padded unit
// therefore has u = tanh(0) = 0 and (by induction from the leaves, whose c = 0) c = 0.5 c_l + 0.5 c_r = 0 and h = 0,
// and zero weight columns keep it out of every K sum; in the backward its dh, dc and gate gradients are 0 for the
// same reason. So the cell needs no special case. Only the module's own tensors have width H: the output and
// gradOutput are guarded by `j < H`; the biases are read from their packed, padded copies.
//
// Forward, workgroup = 16 hidden units (16 * NG gate rows of W, row = unit * NG + gate) x 16 rows of the level, 4
// waves taking the k-steps round-robin; the NG gate partials of a (row, unit) pair meet in LDS and the cell runs
// coalesced along the hidden dimension. Backward, workgroup = 16 rows x 16 units: dh = gradOutput[node] +
// dg16[parent slot] . W_side (K = NG * Hp, gate-major), then the cell backward emits dg (fp32 for the bias sums, bf16
// for the next launches and the weight-gradient GEMMs) at the node's slot.
#include <vector>

#include "common.h"
#include "kernels.h"
#include "rnn_step.h"

namespace {

constexpr int TW = 8;      // ints per table row
struct Row { int node, slot, pslot, side, xrow; };
__device__ __forceinline__ Row load_row(const int* __restrict__ tab, int row) {
  const int* e = tab + (long)row * TW;
  return Row{e[0], e[1], e[2], e[3], e[4]};
}

// Leaves: bf16 input rows by leaf slot, zero-padded to Ip: the leaf GEMM's operand and dW_leaf's.
__global__ void __launch_bounds__(64) treelstm_gather_x_kernel(const float* __restrict__ x, const int* __restrict__ tab,
                                                               bf16_t* __restrict__ xl16, int I, int Ip) {
  const Row e = load_row(tab, blockIdx.x);
  if (e.node < 0) return;
  for (int k = threadIdx.x; k < Ip; k += 64)
    xl16[(long)e.slot * Ip + k] = k < I ? f2bf(x[(long)e.xrow * I + k]) : (bf16_t)0;
}

// Forward level. NG gate blocks (composer 5 / 4, leaf 2 / 1); src16 rows by own slot, K wide (hch16, K = 2 Hp; xl16,
// K = Ip). acts: composer [slot][NG + 1][Hp] = gates in weight order then tanh(c); leaf [slot][NG][Hp] = tanh(c), o.
template <int NG, bool LEAF>
__global__ void __launch_bounds__(256) treelstm_fwd_level_kernel(
    const bf16_t* __restrict__ W16, const bf16_t* __restrict__ src16, const float* __restrict__ bias,
    const int* __restrict__ tab, float* __restrict__ cch, bf16_t* __restrict__ hch16, float* __restrict__ out,
    float* __restrict__ acts, int H, int Hp, int K, int Z) {
  __shared__ float gl[4][16][16 * NG + 1];                   // [k wave][row][unit * NG + gate]
  const int lane = threadIdx.x & 63, kc = threadIdx.x >> 6;
  const int r = lane & 15, kh = lane >> 4;
  const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  const int m = threadIdx.x >> 4, n = threadIdx.x & 15, j = j0 + n;
  const Row e = load_row(tab, m0 + m);
  float lc = 0.f, rc = 0.f, bg[NG];
  if constexpr (!LEAF) {                                     // cell operands in flight while the GEMM runs
    lc = cch[(long)e.slot * 2 * Hp + j];
    rc = cch[(long)e.slot * 2 * Hp + Hp + j];
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) bg[g] = bias[j * NG + g];
  {
    v4f acc[NG];
#pragma unroll
    for (int mt = 0; mt < NG; ++mt) acc[mt] = v4f{0.f, 0.f, 0.f, 0.f};
    const bf16_t* pw = W16 + (long)(j0 * NG + r) * K + kh * 8;
    const bf16_t* pv = src16 + (long)tab[(long)(m0 + r) * TW + 1] * K + kh * 8;
    const int steps = K / 32;
    for (int s = kc; s < steps; s += 4) {
      v8s a[NG];
#pragma unroll
      for (int mt = 0; mt < NG; ++mt) a[mt] = ld8(pw + (long)mt * 16 * K + s * 32);
      const v8s v = ld8(pv + s * 32);
#pragma unroll
      for (int mt = 0; mt < NG; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], v, acc[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < NG; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) gl[kc][r][mt * 16 + kh * 4 + i] = acc[mt][i];   // D[unit * NG + gate][row]
  }
  __syncthreads();
  if (e.node < 0) return;
  float g[NG];
#pragma unroll
  for (int q = 0; q < NG; ++q) g[q] = bg[q] + ((gl[0][m][n * NG + q] + gl[1][m][n * NG + q]) +
                                              (gl[2][m][n * NG + q] + gl[3][m][n * NG + q]));
  float c, tc, h;
  if constexpr (LEAF) {
    float* a = acts + (long)e.slot * NG * Hp + j;
    c = g[0];
    tc = tanh_f(c);
    a[0] = tc;
    h = tc;
    if constexpr (NG == 2) {
      const float og = sigm(g[1]);
      a[Hp] = og;
      h = og * tc;
    }
  } else {
    float* a = acts + (long)e.slot * (NG + 1) * Hp + j;
    const float ig = sigm(g[0]), lf = sigm(g[1]), rf = sigm(g[2]), ug = tanh_f(g[3]);
    c = ig * ug + lf * lc + rf * rc;
    tc = tanh_f(c);
    a[0] = ig; a[Hp] = lf; a[2 * Hp] = rf; a[3 * Hp] = ug;
    h = tc;
    if constexpr (NG == 5) {
      const float og = sigm(g[4]);
      a[4 * Hp] = og;
      h = og * tc;
    }
    a[(long)NG * Hp] = tc;
  }
  if (j < H) out[(long)e.node * H + j] = h;
  if (e.pslot != Z) {                                        // a root has no parent row to fill
    const long p = (long)e.pslot * 2 * Hp + e.side * Hp + j;
    cch[p] = c;
    hch16[p] = f2bf(h);
  }
}

// Backward level. dg16p: the composers' bf16 gate gradients by slot, K = NGP * Hp wide (gate-major); WT16 [2][Hp][K] =
// W_left^T, W_right^T. Rows [0, split) of the level hang on the left, the rest on the right. GO: the output gate exists.
template <bool LEAF, bool GO>
__global__ void __launch_bounds__(256) treelstm_bwd_level_kernel(
    const bf16_t* __restrict__ WT16, const bf16_t* __restrict__ dg16p, const float* __restrict__ gout,
    const int* __restrict__ tab, int split, const float* __restrict__ acts, const float* __restrict__ cch,
    float* __restrict__ dcp, float* __restrict__ dg, bf16_t* __restrict__ dg16, int H, int Hp, int K, int Z) {
  __shared__ float red[4][16][17];                           // [k wave][row][unit]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kh = lane >> 4;
  const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  const int m = threadIdx.x >> 4, n = threadIdx.x & 15, j = j0 + n;
  const int tside = m0 < split ? 0 : 1;
  const Row e = load_row(tab, m0 + m);
  constexpr int NG = LEAF ? (GO ? 2 : 1) : (GO ? 5 : 4);
  constexpr int NA = LEAF ? NG : NG + 1;
  // cell operands in flight while the GEMM runs (padding rows read slot Z / leaf slot 0 and never store)
  float dh = (e.node >= 0 && j < H) ? gout[(long)e.node * H + j] : 0.f;
  const float dcin = dcp[(long)e.pslot * 2 * Hp + tside * Hp + j];
  float av[NA], lc = 0.f, rc = 0.f;
  const float* a = acts + (long)e.slot * NA * Hp + j;
#pragma unroll
  for (int q = 0; q < NA; ++q) av[q] = a[(long)q * Hp];
  if constexpr (!LEAF) {
    lc = cch[(long)e.slot * 2 * Hp + j];
    rc = cch[(long)e.slot * 2 * Hp + Hp + j];
  }
  {
    v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
    const bf16_t* pa = dg16p + (long)tab[(long)(m0 + r) * TW + 2] * K + kh * 8;
    const bf16_t* pw = WT16 + ((long)tside * Hp + j0 + r) * K + kh * 8;
    const int steps = K / 32;
    for (int s = wave; s < steps; s += 4)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ld8(pa + s * 32), ld8(pw + s * 32), acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][kh * 4 + i][r] = acc[i];               // D[row][unit]
  }
  __syncthreads();
  if (e.node < 0) return;
  dh += (red[0][m][n] + red[1][m][n]) + (red[2][m][n] + red[3][m][n]);
  if constexpr (LEAF) {
    const float tc = av[0], og = GO ? av[1] : 1.f;
    const float dc = dcin + dh * og * (1.f - tc * tc);
    const long o = (long)e.slot * NG * Hp + j;
    dg[o] = dc;
    dg16[o] = f2bf(dc);
    if constexpr (GO) {
      const float dog = dh * tc * og * (1.f - og);
      dg[o + Hp] = dog;
      dg16[o + Hp] = f2bf(dog);
    }
  } else {
    const float ig = av[0], lf = av[1], rf = av[2], ug = av[3], og = GO ? av[4] : 1.f, tc = av[NG];
    const float dc = dcin + dh * og * (1.f - tc * tc);
    const float di = dc * ug * ig * (1.f - ig), dlf = dc * lc * lf * (1.f - lf), drf = dc * rc * rf * (1.f - rf);
    const float du = dc * ig * (1.f - ug * ug);
    dcp[(long)e.slot * 2 * Hp + j] = dc * lf;                // what the left / right child reads as its dcin
    dcp[(long)e.slot * 2 * Hp + Hp + j] = dc * rf;
    const long o = (long)e.slot * NG * Hp + j;
    dg[o] = di; dg[o + Hp] = dlf; dg[o + 2 * Hp] = drf; dg[o + 3 * Hp] = du;
    dg16[o] = f2bf(di); dg16[o + Hp] = f2bf(dlf); dg16[o + 2 * Hp] = f2bf(drf); dg16[o + 3 * Hp] = f2bf(du);
    if constexpr (GO) {
      const float dog = dh * tc * og * (1.f - og);
      dg[o + 4 * Hp] = dog;
      dg16[o + 4 * Hp] = f2bf(dog);
    }
  }
}

// Bias gradients: out[C] = column sums of the fp32 gate gradients a [R][C]. Stage 1: workgroup = 64 columns x 4 row
// lanes over a 64-row slice, each lane in ascending row order, lanes added in lane order; stage 2 adds the slices in
// order. No atomics.
constexpr int CS_ROWS = 64;
__global__ void __launch_bounds__(256) treelstm_colsum_part_kernel(const float* __restrict__ a, float* __restrict__ part,
                                                                   int R, int C) {
  __shared__ float red[4][64];
  const int n = threadIdx.x & 63, y = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + n;
  const int lo = blockIdx.y * CS_ROWS, hi = lo + CS_ROWS < R ? lo + CS_ROWS : R;
  float s = 0.f;
  if (col < C)
    for (int row = lo + y; row < hi; row += 4) s += a[(long)row * C + col];
  red[y][n] = s;
  __syncthreads();
  if (y == 0 && col < C) part[(long)blockIdx.y * C + col] = (red[0][n] + red[1][n]) + (red[2][n] + red[3][n]);
}
__global__ void __launch_bounds__(256) treelstm_colsum_sum_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                  int S, int C) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= C) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += part[(long)s * C + col];
  out[col] = v;
}

// gradInput row (b, word) = sum of dx over the leaves that name the word, in leaf-slot order (off / items: the
// schedule's CSR lists); a word no leaf names gets 0. Every element of gin is written once.
__global__ void __launch_bounds__(64) treelstm_leaf_dx_kernel(const float* __restrict__ dxl, const int* __restrict__ off,
                                                              const int* __restrict__ items, float* __restrict__ gin,
                                                              int I, int Ip) {
  const int lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
  for (int k = threadIdx.x; k < I; k += 64) {
    float v = 0.f;
    for (int q = lo; q < hi; ++q) v += dxl[(long)items[q] * Ip + k];
    gin[(long)blockIdx.x * I + k] = v;
  }
}

struct Nd { int node, parent, side, height, xrow, slot, kid[2]; };
struct Frame { int n, idx, stage; };

}  // namespace

int bigdl_treelstm_schedule(const int64_t* trees, int B, int N, int L, std::vector<int32_t>& tab,
                            std::vector<int64_t>& meta) {
  tab.clear();
  meta.clear();
  if (B < 1 || N < 1 || L < 1 || (long)B * N >= (1L << 30) || (long)B * L >= (1L << 30)) return -1;
  std::vector<Nd> nodes;
  std::vector<char> seen(N);
  std::vector<Frame> stack;
  int maxh = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* t = trees + (long)b * N * 3;
    int root = -1;
    for (int n = 0; n < N; ++n) {
      if (t[n * 3 + 2] != -1) continue;
      if (t[n * 3] == -1) {            // a padding row; before the root it is what the loop would start from
        if (root < 0) return -1;
        continue;
      }
      if (root >= 0) return -1;        // two roots
      root = n;
    }
    if (root < 0) return -1;
    std::fill(seen.begin(), seen.end(), 0);
    seen[root] = 1;
    nodes.push_back(Nd{b * N + root, -1, 0, 0, 0, 0, {-1, -1}});
    stack.push_back(Frame{root, (int)nodes.size() - 1, 0});
    while (!stack.empty()) {
      Frame& f = stack.back();
      const int64_t c0 = t[f.n * 3], c1 = t[f.n * 3 + 1], tag = t[f.n * 3 + 2];
      if (f.stage == 1) {
        const int hl = nodes[nodes[f.idx].kid[0]].height, hr = nodes[nodes[f.idx].kid[1]].height;
        nodes[f.idx].height = 1 + (hl > hr ? hl : hr);
        if (nodes[f.idx].height > maxh) maxh = nodes[f.idx].height;
        stack.pop_back();
        continue;
      }
      if (c0 == 0) {                   // leaf; a word index below 1 counts from the end, as the loop's indexing does
        int64_t w = tag - 1;
        if (w < 0) w += L;
        if (w < 0 || w >= L) return -1;
        nodes[f.idx].xrow = (int)((long)b * L + w);
        stack.pop_back();
        continue;
      }
      if (c0 < 1 || c0 > N || c1 < 1 || c1 > N) return -1;
      f.stage = 1;
      const int idx = f.idx;           // f dangles once the stack grows
      const int kids[2] = {(int)c0 - 1, (int)c1 - 1};
      for (int s = 0; s < 2; ++s) {
        if (seen[kids[s]] || t[kids[s] * 3] == -1) return -1;      // a second parent, a cycle, or a padding row
        seen[kids[s]] = 1;
        nodes.push_back(Nd{b * N + kids[s], idx, s, 0, 0, 0, {-1, -1}});
        nodes[idx].kid[s] = (int)nodes.size() - 1;
      }
      stack.push_back(Frame{kids[1], nodes[idx].kid[1], 0});
      stack.push_back(Frame{kids[0], nodes[idx].kid[0], 0});
    }
  }
  // slots: composers level by level (left group, then right group), leaves likewise
  const int nlev = maxh + 1;
  std::vector<std::vector<int>> group(2 * nlev);
  for (int i = 0; i < (int)nodes.size(); ++i) group[nodes[i].height * 2 + nodes[i].side].push_back(i);
  int S = 0, Lc = 0;
  for (int k = 0; k < nlev; ++k)
    for (int s = 0; s < 2; ++s)
      for (int i : group[k * 2 + s]) nodes[i].slot = k == 0 ? Lc++ : S++;
  const int Z = S;
  long rows = 0;
  std::vector<int64_t> lv;
  for (int k = 0; k < nlev; ++k) {
    const long start = rows;
    long split = rows;
    for (int s = 0; s < 2; ++s) {
      for (int i : group[k * 2 + s]) {
        const Nd& nd = nodes[i];
        const int row[TW] = {nd.node, nd.slot, nd.parent < 0 ? Z : nodes[nd.parent].slot, s, nd.xrow, 0, 0, 0};
        tab.insert(tab.end(), row, row + TW);
        ++rows;
      }
      for (; rows % 16; ++rows) {
        const int row[TW] = {-1, k == 0 ? 0 : Z, Z, s, 0, 0, 0, 0};
        tab.insert(tab.end(), row, row + TW);
      }
      if (s == 0) split = rows;
    }
    lv.push_back(start); lv.push_back(split); lv.push_back(rows);
  }
  // words -> leaf slots
  const long off0 = (long)tab.size();
  std::vector<int32_t> off((long)B * L + 1, 0);
  for (int i : group[0]) ++off[nodes[i].xrow + 1];
  for (int i : group[1]) ++off[nodes[i].xrow + 1];
  for (long w = 0; w < (long)B * L; ++w) off[w + 1] += off[w];
  std::vector<int32_t> items(Lc), fill(off.begin(), off.end() - 1);
  std::vector<int> byslot(Lc);
  for (int s = 0; s < 2; ++s)
    for (int i : group[s]) byslot[nodes[i].slot] = i;
  for (int q = 0; q < Lc; ++q) items[fill[nodes[byslot[q]].xrow]++] = q;
  tab.insert(tab.end(), off.begin(), off.end());
  const long items0 = (long)tab.size();
  tab.insert(tab.end(), items.begin(), items.end());
  meta = {S, Lc, nlev, rows, off0, items0};
  meta.insert(meta.end(), lv.begin(), lv.end());
  return 0;
}

int bigdl_treelstm_gather_x(const float* x, const int* tab, int rows, uint16_t* xl16, int I, int Ip, hipStream_t st) {
  if (rows <= 0 || I <= 0 || Ip % 32 != 0 || Ip < I) return -1;
  treelstm_gather_x_kernel<<<rows, 64, 0, st>>>(x, tab, xl16, I, Ip);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_treelstm_fwd_level(const uint16_t* W16, const uint16_t* src16, const float* bias, const int* tab, int rows,
                             float* cch, uint16_t* hch16, float* out, float* acts, int H, int Hp, int K, int Z, int ng,
                             int leaf, hipStream_t st) {
  if (rows <= 0 || rows % 16 != 0 || H <= 0 || Hp % 32 != 0 || Hp < H || K <= 0 || K % 32 != 0) return -1;
  if (leaf ? (ng != 1 && ng != 2) : (ng != 4 && ng != 5)) return -1;
  const auto kernel = leaf ? (ng == 2 ? treelstm_fwd_level_kernel<2, true> : treelstm_fwd_level_kernel<1, true>)
                           : (ng == 5 ? treelstm_fwd_level_kernel<5, false> : treelstm_fwd_level_kernel<4, false>);
  kernel<<<dim3(Hp / 16, rows / 16), 256, 0, st>>>(W16, src16, bias, tab, cch, hch16, out, acts, H, Hp, K, Z);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_treelstm_bwd_level(const uint16_t* WT16, const uint16_t* dg16p, const float* gout, const int* tab, int split,
                             int rows, const float* acts, const float* cch, float* dcp, float* dg, uint16_t* dg16,
                             int H, int Hp, int K, int Z, int gate_output, int leaf, hipStream_t st) {
  if (rows <= 0 || rows % 16 != 0 || split < 0 || split > rows || split % 16 != 0) return -1;
  if (H <= 0 || Hp % 32 != 0 || Hp < H || K != (gate_output ? 5 : 4) * Hp) return -1;
  const auto kernel = leaf ? (gate_output ? treelstm_bwd_level_kernel<true, true> : treelstm_bwd_level_kernel<true, false>)
                           : (gate_output ? treelstm_bwd_level_kernel<false, true> : treelstm_bwd_level_kernel<false, false>);
  kernel<<<dim3(Hp / 16, rows / 16), 256, 0, st>>>(WT16, dg16p, gout, tab, split, acts, cch, dcp, dg, dg16, H, Hp, K, Z);
  HIP_LAUNCH_CHECK();
  return 0;
}

long bigdl_treelstm_colsum_ws(int R, int C) { return (long)((R + CS_ROWS - 1) / CS_ROWS) * C; }

int bigdl_treelstm_colsum(const float* a, float* part, float* out, int R, int C, hipStream_t st) {
  if (R <= 0 || C <= 0) return -1;
  const int S = (R + CS_ROWS - 1) / CS_ROWS;
  treelstm_colsum_part_kernel<<<dim3((C + 63) / 64, S), 256, 0, st>>>(a, part, R, C);
  HIP_LAUNCH_CHECK();
  treelstm_colsum_sum_kernel<<<(C + 255) / 256, 256, 0, st>>>(part, out, S, C);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_treelstm_leaf_dx(const float* dxl, const int* off, const int* items, float* gin, int words, int I, int Ip,
                           hipStream_t st) {
  if (words <= 0 || I <= 0 || Ip < I) return -1;
  treelstm_leaf_dx_kernel<<<words, 64, 0, st>>>(dxl, off, items, gin, I, Ip);
  HIP_LAUNCH_CHECK();
  return 0;
}
