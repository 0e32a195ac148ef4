// Sparse (COO) kernels of the wide half of Wide & Deep models, for gfx950.
//
// Reference counterparts:
//   SparseLinear        S/nn/SparseLinear.scala:60 (fwd), :84 (bwd window), :102 (bwd weight)
//                       S/tensor/SparseTensorMath.scala addmm
//   LookupTableSparse   S/nn/LookupTableSparse.scala:77 (fwd), :166 (bwd weight)
//   SparseJoinTable     S/nn/SparseJoinTable.scala, S/tensor/SparseTensor.scala sparseConcat
//
// The input is a coalesced 2-D COO tensor as torch stores it: int64 rows[nnz] and cols[nnz] in row-major order, fp32
// values. coo_row_offsets turns the sorted rows into int32 CSR offsets [B + 1] once per tensor; the forward kernels
// and the join read row segments through them, the per-entry gradient kernels take the entry's own row index.
//
// Rules every kernel here keeps:
// * no index is used as an address before it is range-checked: a row outside [0, B), a column outside [0, D) or an id
//   outside [1, nIndex] contributes nothing (the offsets exclude rows outside [0, B) by construction);
// * nothing is sized by B * D, and nothing waits on the host;
// * an empty call (nnz == 0) is answered by the caller: no launch from this file.
//
// Design notes (MI355X):
// * spmm forward. The regime is D >> nnz per row (tens of entries) and N from 1 to a few hundred, W as stored [N, D].
//   A gather of W[o, col] is one 4-byte read per (entry, output) whichever way the lanes are laid, so the mapping is
//   chosen for lane occupancy. N <= 8: a 16-lane group per row with the lanes over the row's entries, one register
//   accumulator per output and a fixed xor-fold (8, 4, 2, 1) inside the group: four rows per wave and no idle lanes
//   at 16+ entries per row, where lanes over two outputs would leave 62 of 64 idle. N > 8: a wave per (row, 64-output
//   slice), lanes over outputs, each lane walking the row in stored order. Both orders are a function of the row's
//   length alone, so the forward is bitwise reproducible.
// * weight gradients. nnz * N fp32 atomics straight into gradWeight, a thread per (entry, output) with the output
//   fastest so gy is read coalesced. With W stored [N, D] the adds of one entry land D floats apart, one lane per
//   row: the slow shape for float atomics, but the whole scatter is nnz * N * 4 bytes (1.3 MB at batch 8192 with 40
//   entries per row and N = 2), far below what the chip adds per second in any shape. LookupTableSparse's scatter
//   has lanes along nOutput: 256 contiguous bytes per wave instruction. Deterministic mode: the caller sorts the entries stably by column / id; the
//   thread whose slot opens a run sums the run in order and stores once (as embedding_bwd_sorted_kernel does).
// * LookupTableSparse. A wave per (row, 64-column slice), lanes along nOutput: every gathered weight row is one
//   coalesced 256-byte read per wave.
#include "common.h"
#include "kernels.h"

namespace {

#define GS_LOOP(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

constexpr int GROUP = 16;      // lanes per row group (spmm forward for small N, sddmm for large N, join)
constexpr int NSMALL = 8;      // largest N on the lanes-over-entries mapping

inline int blocks_for(long work, int threads = 256, int cap = 16384) {
  long g = (work + threads - 1) / threads;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------ CSR offsets
// offs[b] = first entry whose row is >= b (lower bound), b in [0, B]: entries of rows < 0 sit before offs[0] and
// entries of rows >= B after offs[B], so no segment contains them.
__global__ void coo_row_offsets_kernel(const long* __restrict__ rows, int nnz, int B, int* __restrict__ offs) {
  GS_LOOP(b, (long)B + 1) {
    int lo = 0, hi = nnz;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (rows[mid] < b) lo = mid + 1; else hi = mid;
    }
    offs[b] = lo;
  }
}

// ------------------------------------------------------------------------------------------ spmm forward
__global__ void spmm_fwd_entries_kernel(const long* __restrict__ cols, const float* __restrict__ vals,
                                        const int* __restrict__ offs, const float* __restrict__ W,
                                        const float* __restrict__ bias, float* __restrict__ y, int B, int N, long D) {
  const int sub = threadIdx.x & (GROUP - 1);
  const long gid = (blockIdx.x * (long)blockDim.x + threadIdx.x) / GROUP;
  const long ng = ((long)gridDim.x * blockDim.x) / GROUP;
  for (long b = gid; b < B; b += ng) {
    const int lo = offs[b], hi = offs[b + 1];
    float acc[NSMALL];
#pragma unroll
    for (int o = 0; o < NSMALL; ++o) acc[o] = 0.f;
    for (int k = lo + sub; k < hi; k += GROUP) {
      const long c = cols[k];
      if (c < 0 || c >= D) continue;
      const float v = vals[k];
#pragma unroll
      for (int o = 0; o < NSMALL; ++o)
        if (o < N) acc[o] += v * W[o * D + c];
    }
#pragma unroll
    for (int o = 0; o < NSMALL; ++o) acc[o] = group_sum(acc[o]);
    if (sub == 0) {
#pragma unroll
      for (int o = 0; o < NSMALL; ++o)
        if (o < N) y[b * N + o] = (bias ? bias[o] : 0.f) + acc[o];
    }
  }
}

__global__ void spmm_fwd_outputs_kernel(const long* __restrict__ cols, const float* __restrict__ vals,
                                        const int* __restrict__ offs, const float* __restrict__ W,
                                        const float* __restrict__ bias, float* __restrict__ y, int B, int N, long D) {
  const int lane = threadIdx.x & 63;
  const long wid = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  const long slices = (N + 63) / 64;
  for (long w = wid; w < B * slices; w += nw) {
    const long b = w / slices;
    const int o = (int)(w % slices) * 64 + lane;
    if (o >= N) continue;
    const int lo = offs[b], hi = offs[b + 1];
    const float* wo = W + o * D;
    float acc = 0.f;
    for (int k = lo; k < hi; ++k) {
      const long c = cols[k];
      if (c < 0 || c >= D) continue;
      acc += vals[k] * wo[c];
    }
    y[b * N + o] = (bias ? bias[o] : 0.f) + acc;
  }
}

// ------------------------------------------------------------------------------------------ spmm weight gradient
__global__ void spmm_wgrad_atomic_kernel(const long* __restrict__ rows, const long* __restrict__ cols,
                                         const float* __restrict__ vals, const float* __restrict__ gy,
                                         float* __restrict__ gW, long nnz, int B, int N, long D, float scale) {
  GS_LOOP(i, nnz * N) {
    const long k = i / N;
    const int o = (int)(i - k * N);
    const long r = rows[k], c = cols[k];
    if (r < 0 || r >= B || c < 0 || c >= D) continue;
    atomicAdd(gW + o * D + c, scale * (vals[k] * gy[r * N + o]));
  }
}

// keys = the entries' columns stably sorted (entries to skip carry -1), pos = the matching entry numbers
__global__ void spmm_wgrad_sorted_kernel(const long* __restrict__ keys, const long* __restrict__ pos,
                                         const long* __restrict__ rows, const float* __restrict__ vals,
                                         const float* __restrict__ gy, float* __restrict__ gW, long nnz, int B, int N,
                                         long D, float scale) {
  GS_LOOP(i, nnz * N) {
    const long s = i / N;
    const int o = (int)(i - s * N);
    const long c = keys[s];
    if (c < 0 || c >= D || (s > 0 && keys[s - 1] == c)) continue;
    float sum = 0.f;
    for (long j = s; j < nnz && keys[j] == c; ++j) {
      const long p = pos[j];
      if (p < 0 || p >= nnz) continue;
      const long r = rows[p];
      if (r < 0 || r >= B) continue;
      sum += vals[p] * gy[r * N + o];
    }
    gW[o * D + c] += scale * sum;
  }
}

// ------------------------------------------------------------------------------------------ sddmm on the input's pattern
// g[k] = sum_o gy[row_k, o] * W[o, col_k]; G lanes per entry over the outputs (G = 1: a thread per entry)
template <int G>
__global__ void sddmm_rows_kernel(const long* __restrict__ rows, const long* __restrict__ cols,
                                  const float* __restrict__ gy, const float* __restrict__ W, float* __restrict__ g,
                                  long nnz, int B, int N, long D) {
  const int sub = threadIdx.x & (G - 1);
  const long gid = (blockIdx.x * (long)blockDim.x + threadIdx.x) / G;
  const long ng = ((long)gridDim.x * blockDim.x) / G;
  for (long k = gid; k < nnz; k += ng) {
    const long r = rows[k], c = cols[k];
    float acc = 0.f;
    if (r >= 0 && r < B && c >= 0 && c < D)
      for (int o = sub; o < N; o += G) acc += gy[r * N + o] * W[o * D + c];
    if (G > 1) acc = group_sum(acc);
    if (sub == 0) g[k] = acc;
  }
}

// ------------------------------------------------------------------------------------------ LookupTableSparse
// comb: 0 sum, 1 mean, 2 sqrtn. ids are the fp32 values of the sparse id tensor (1-based), wts the values of the
// weight tensor on the same pattern, or null for w = 1.
__device__ __forceinline__ long lookup_row(const float* ids, int k, long nIndex) {
  const long id = (long)ids[k];
  return (id >= 1 && id <= nIndex) ? id - 1 : -1;
}

__global__ void lookup_sparse_fwd_kernel(const int* __restrict__ offs, const float* __restrict__ ids,
                                         const float* __restrict__ wts, const float* __restrict__ W,
                                         float* __restrict__ out, float* __restrict__ sc, int B, int nOut, long nIndex,
                                         int comb) {
  const int lane = threadIdx.x & 63;
  const long wid = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  const long slices = (nOut + 63) / 64;
  for (long w = wid; w < B * slices; w += nw) {
    const long b = w / slices;
    const int slice = (int)(w % slices);
    const int d = slice * 64 + lane;
    const int lo = offs[b], hi = offs[b + 1];
    float s = 1.f;
    if (comb != 0) {       // every lane folds the same sequence: no exchange, identical s across the row's waves
      float den = 0.f;
      for (int k = lo; k < hi; ++k) {
        if (lookup_row(ids, k, nIndex) < 0) continue;
        const float wk = wts ? wts[k] : 1.f;
        den += comb == 1 ? wk : wk * wk;
      }
      if (comb == 1) s = den != 0.f ? 1.f / den : 0.f;
      else s = den > 0.f ? 1.f / sqrtf(den) : 0.f;
    }
    if (slice == 0 && lane == 0) sc[b] = s;
    if (d >= nOut) continue;
    float acc = 0.f;
    for (int k = lo; k < hi; ++k) {
      const long row = lookup_row(ids, k, nIndex);
      if (row < 0) continue;
      acc += (wts ? wts[k] : 1.f) * W[row * nOut + d];
    }
    out[b * nOut + d] = s * acc;
  }
}

__global__ void lookup_sparse_bwd_atomic_kernel(const int* __restrict__ offs, const float* __restrict__ ids,
                                                const float* __restrict__ wts, const float* __restrict__ sc,
                                                const float* __restrict__ gy, float* __restrict__ gW, int B, int nOut,
                                                long nIndex, float scale) {
  const int lane = threadIdx.x & 63;
  const long wid = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  const long slices = (nOut + 63) / 64;
  for (long w = wid; w < B * slices; w += nw) {
    const long b = w / slices;
    const int d = (int)(w % slices) * 64 + lane;
    if (d >= nOut) continue;
    const int lo = offs[b], hi = offs[b + 1];
    const float t = sc[b] * gy[b * nOut + d];
    for (int k = lo; k < hi; ++k) {
      const long row = lookup_row(ids, k, nIndex);
      if (row < 0) continue;
      atomicAdd(gW + row * nOut + d, scale * ((wts ? wts[k] : 1.f) * t));
    }
  }
}

// keys = the entries' weight rows (id - 1) stably sorted (entries to skip carry -1), pos = the matching entry numbers
__global__ void lookup_sparse_bwd_sorted_kernel(const long* __restrict__ keys, const long* __restrict__ pos,
                                                const long* __restrict__ rows, const float* __restrict__ wts,
                                                const float* __restrict__ sc, const float* __restrict__ gy,
                                                float* __restrict__ gW, long nnz, int B, int nOut, long nIndex,
                                                float scale) {
  const int lane = threadIdx.x & 63;
  const long wid = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  const long slices = (nOut + 63) / 64;
  for (long w = wid; w < nnz * slices; w += nw) {
    const long i = w / slices;
    const int d = (int)(w % slices) * 64 + lane;
    const long key = keys[i];
    if (key < 0 || key >= nIndex || (i > 0 && keys[i - 1] == key) || d >= nOut) continue;
    float sum = 0.f;
    for (long j = i; j < nnz && keys[j] == key; ++j) {
      const long p = pos[j];
      if (p < 0 || p >= nnz) continue;
      const long r = rows[p];
      if (r < 0 || r >= B) continue;
      sum += (wts ? wts[p] : 1.f) * (sc[r] * gy[r * nOut + d]);
    }
    gW[key * nOut + d] += scale * sum;
  }
}

// ------------------------------------------------------------------------------------------ join along the columns
// Output row b = the inputs' row-b segments in input order, columns shifted by the widths before: a 16-lane group per
// row copies segment after segment, so the result is row-major sorted by construction.
__global__ void sparse_concat_cols_kernel(SparseJoinInputs in, int B, long* __restrict__ out_rows,
                                          long* __restrict__ out_cols, float* __restrict__ out_vals, long total) {
  const int sub = threadIdx.x & (GROUP - 1);
  const long gid = (blockIdx.x * (long)blockDim.x + threadIdx.x) / GROUP;
  const long ng = ((long)gridDim.x * blockDim.x) / GROUP;
  for (long b = gid; b < B; b += ng) {
    long base = 0;
    for (int i = 0; i < in.n; ++i) base += in.offs[i][b] - in.offs[i][0];
    for (int i = 0; i < in.n; ++i) {
      const int lo = in.offs[i][b], hi = in.offs[i][b + 1];
      for (int k = lo + sub; k < hi; k += GROUP) {
        const long p = base + (k - lo);
        if (p >= total) continue;
        out_rows[p] = b;
        out_cols[p] = in.cols[i][k] + in.shift[i];
        out_vals[p] = in.vals[i][k];
      }
      base += hi - lo;
    }
  }
}

}  // namespace

// ============================================================================================ C ABI
void bigdl_coo_row_offsets(const long* rows, long nnz, int B, int* offs, hipStream_t st) {
  coo_row_offsets_kernel<<<blocks_for((long)B + 1), 256, 0, st>>>(rows, (int)nnz, B, offs);
  HIP_LAUNCH_CHECK();
}

void bigdl_spmm_fwd(const long* cols, const float* vals, const int* offs, const float* W, const float* bias, float* y,
                    int B, int N, long D, hipStream_t st) {
  if (B <= 0 || N <= 0) return;
  if (N <= NSMALL)
    spmm_fwd_entries_kernel<<<blocks_for((long)B * GROUP), 256, 0, st>>>(cols, vals, offs, W, bias, y, B, N, D);
  else
    spmm_fwd_outputs_kernel<<<blocks_for((long)B * ((N + 63) / 64) * 64), 256, 0, st>>>(cols, vals, offs, W, bias, y,
                                                                                         B, N, D);
  HIP_LAUNCH_CHECK();
}

void bigdl_spmm_wgrad(const long* rows, const long* cols, const float* vals, const float* gy, float* gW, long nnz,
                      int B, int N, long D, float scale, hipStream_t st) {
  if (nnz <= 0 || N <= 0) return;
  spmm_wgrad_atomic_kernel<<<blocks_for(nnz * N), 256, 0, st>>>(rows, cols, vals, gy, gW, nnz, B, N, D, scale);
  HIP_LAUNCH_CHECK();
}

void bigdl_spmm_wgrad_sorted(const long* keys, const long* pos, const long* rows, const float* vals, const float* gy,
                             float* gW, long nnz, int B, int N, long D, float scale, hipStream_t st) {
  if (nnz <= 0 || N <= 0) return;
  spmm_wgrad_sorted_kernel<<<blocks_for(nnz * N), 256, 0, st>>>(keys, pos, rows, vals, gy, gW, nnz, B, N, D, scale);
  HIP_LAUNCH_CHECK();
}

void bigdl_sddmm_rows(const long* rows, const long* cols, const float* gy, const float* W, float* g, long nnz, int B,
                      int N, long D, hipStream_t st) {
  if (nnz <= 0) return;
  if (N <= NSMALL)
    sddmm_rows_kernel<1><<<blocks_for(nnz), 256, 0, st>>>(rows, cols, gy, W, g, nnz, B, N, D);
  else
    sddmm_rows_kernel<GROUP><<<blocks_for(nnz * GROUP), 256, 0, st>>>(rows, cols, gy, W, g, nnz, B, N, D);
  HIP_LAUNCH_CHECK();
}

void bigdl_lookup_sparse_fwd(const int* offs, const float* ids, const float* wts, const float* W, float* out,
                             float* scales, int B, int nOut, long nIndex, int combiner, hipStream_t st) {
  if (B <= 0 || nOut <= 0) return;
  lookup_sparse_fwd_kernel<<<blocks_for((long)B * ((nOut + 63) / 64) * 64), 256, 0, st>>>(offs, ids, wts, W, out,
                                                                                           scales, B, nOut, nIndex,
                                                                                           combiner);
  HIP_LAUNCH_CHECK();
}

void bigdl_lookup_sparse_bwd(const int* offs, const float* ids, const float* wts, const float* scales, const float* gy,
                             float* gW, int B, int nOut, long nIndex, float scale, hipStream_t st) {
  if (B <= 0 || nOut <= 0) return;
  lookup_sparse_bwd_atomic_kernel<<<blocks_for((long)B * ((nOut + 63) / 64) * 64), 256, 0, st>>>(
      offs, ids, wts, scales, gy, gW, B, nOut, nIndex, scale);
  HIP_LAUNCH_CHECK();
}

void bigdl_lookup_sparse_bwd_sorted(const long* keys, const long* pos, const long* rows, const float* wts,
                                    const float* scales, const float* gy, float* gW, long nnz, int B, int nOut,
                                    long nIndex, float scale, hipStream_t st) {
  if (nnz <= 0 || nOut <= 0) return;
  lookup_sparse_bwd_sorted_kernel<<<blocks_for(nnz * ((nOut + 63) / 64) * 64), 256, 0, st>>>(
      keys, pos, rows, wts, scales, gy, gW, nnz, B, nOut, nIndex, scale);
  HIP_LAUNCH_CHECK();
}

int bigdl_sparse_concat_cols(const SparseJoinInputs* in, int B, long* out_rows, long* out_cols, float* out_vals,
                             long total, hipStream_t st) {
  if (in->n < 1 || in->n > BIGDL_SPARSE_MAX_JOIN) return -1;
  if (B <= 0 || total <= 0) return 0;
  sparse_concat_cols_kernel<<<blocks_for((long)B * GROUP), 256, 0, st>>>(*in, B, out_rows, out_cols, out_vals, total);
  HIP_LAUNCH_CHECK();
  return 0;
}
