// Single-token attention decode over a preallocated KV cache, and the two cache maintenance kernels of incremental
// beam search (bigdl_amd/nn/transformer.py _DecodeState).
//
//   attn_decode   o[n][h*D..] = softmax(q[n][h] . K[row(n)][0..len)[h] + bias[row(n)][0..len)) V[row(n)][0..len)[h]
//   kv_append     this step's fp32 K and V rows -> position pos of both bf16 caches, one launch
//   kv_reorder    dst[x][n][0..len) = src[x][parent[n]][0..len) for every (layer, k/v) plane x, one launch
//
// attn_decode is the memory-bound kernel type: one query row per (sequence, head), so there is no MFMA tile and no
// LDS staging; K and V go straight from HBM to registers. One 256-thread workgroup per (sequence, head). A key's D
// bf16 values are spread over G = 4 / 8 / 16 / 16 lanes (D = 32 / 64 / 96 / 128; at D = 96 lanes 12..15 of a group
// idle), 16 bytes per lane, so a wave covers 64 / G keys per pass and the workgroup's four waves 256 / G keys
// (64 / 32 / 16 / 16). The dot product is reduced over the G lanes with xor shuffles; each lane group keeps an fp32
// online softmax (running max, sum, and its 8 output columns), the groups of a wave are folded with shuffles and the
// four waves once through LDS. q is rounded to bf16 on load (round to nearest even), the operands the flash kernel
// sees for the same step; scores, softmax and P.V stay fp32 and P is never rounded.
//
// No split of the key range across workgroups: decode lengths here are tens to hundreds of keys (maxDecodeLength,
// source sentence length), a handful of passes per workgroup, and B * beam * heads workgroups already fill the chip.
//
// Memory safety: keys >= len are never loaded (their lanes carry score -inf and weight 0), len <= Lmax is checked by
// the host entry, and a cache row index outside [0, R) is clamped, so neither a stale cache tail nor a bad row map
// can reach the result or fault. A row whose keys all carry -inf gives 0 (the flash kernel's pinned behaviour); a
// row whose keys all carry -1e9 gives the uniform average, as the fp32 add absorbs the scores.
#include "common.h"
#include "kernels.h"

#define AD_THREADS 256
#define AD_WAVES (AD_THREADS / WAVE)

namespace {

struct Soft {
  float m, l;
  float acc[8];
};

// fold b into a (two partial online softmaxes over disjoint key sets)
__device__ __forceinline__ void soft_merge(Soft& a, float bm, float bl, const float* bacc) {
  const float M = fmaxf(a.m, bm);
  if (M == -INFINITY) return;                      // both empty: stay (m = -inf, l = 0, acc = 0)
  const float wa = __expf(a.m - M), wb = __expf(bm - M);
  a.l = a.l * wa + bl * wb;
#pragma unroll
  for (int e = 0; e < 8; ++e) a.acc[e] = a.acc[e] * wa + bacc[e] * wb;
  a.m = M;
}

template <int D, int G>
__global__ __launch_bounds__(AD_THREADS) void attn_decode_kernel(const float* __restrict__ q,
                                                                 const bf16_t* __restrict__ kc,
                                                                 const bf16_t* __restrict__ vc,
                                                                 const int* __restrict__ rows,
                                                                 const float* __restrict__ bias, float* __restrict__ o,
                                                                 int R, int Lmax, int hidden, int len) {
  constexpr int KPW = WAVE / G;                    // keys per wave pass
  constexpr int KPB = KPW * AD_WAVES;              // keys per workgroup pass
  const int n = blockIdx.x, h = blockIdx.y;
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const int sub = lane % G, grp = lane / G;
  const bool live = sub * 8 < D;                   // D = 96: lanes 12..15 of a group hold no columns
  int r = rows ? rows[n] : n;
  r = min(max(r, 0), R - 1);

  float qf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] = 0.f;
  if (live) {
    const float* qp = q + (long)n * hidden + h * D + sub * 8;
    const v4f a = *reinterpret_cast<const v4f*>(qp), b = *reinterpret_cast<const v4f*>(qp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qf[e] = bf2f(f2bf(a[e]));
      qf[4 + e] = bf2f(f2bf(b[e]));
    }
  }
  const long base = (long)r * Lmax * hidden + h * D + sub * 8;
  const float* brow = bias ? bias + (long)r * Lmax : nullptr;

  Soft s;
  s.m = -INFINITY;
  s.l = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s.acc[e] = 0.f;

  for (int j0 = 0; j0 < len; j0 += KPB) {
    const int j = j0 + wave * KPW + grp;
    const bool in = j < len;
    v4u kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
    float bj = 0.f;
    if (in && live) {
      const long off = base + (long)j * hidden;
      kk = *reinterpret_cast<const v4u*>(kc + off);
      vv = *reinterpret_cast<const v4u*>(vc + off);
    }
    if (in && brow) bj = brow[j];
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) d += qf[2 * e] * lo_bf(kk[e]) + qf[2 * e + 1] * hi_bf(kk[e]);
#pragma unroll
    for (int x = 1; x < G; x <<= 1) d += __shfl_xor(d, x, 64);
    const float sc = in ? d + bj : -INFINITY;
    const float M = fmaxf(s.m, sc);
    if (M != -INFINITY) {                          // else: nothing seen yet and this key is masked out
      const float w = __expf(s.m - M), p = __expf(sc - M);
      s.l = s.l * w + p;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s.acc[2 * e] = s.acc[2 * e] * w + p * lo_bf(vv[e]);
        s.acc[2 * e + 1] = s.acc[2 * e + 1] * w + p * hi_bf(vv[e]);
      }
      s.m = M;
    }
  }

  // the wave's key groups: lanes with the same sub hold the same columns
#pragma unroll
  for (int x = G; x < WAVE; x <<= 1) {
    float ba[8];
    const float bm = __shfl_xor(s.m, x, 64), bl = __shfl_xor(s.l, x, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) ba[e] = __shfl_xor(s.acc[e], x, 64);
    soft_merge(s, bm, bl, ba);
  }

  __shared__ float sm[AD_WAVES][2];
  __shared__ float sacc[AD_WAVES][G * 8];
  if (lane < G) {
    if (lane == 0) {
      sm[wave][0] = s.m;
      sm[wave][1] = s.l;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sacc[wave][lane * 8 + e] = s.acc[e];
  }
  __syncthreads();
  if (tid < D) {
    float M = sm[0][0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) M = fmaxf(M, sm[w][0]);
    float l = 0.f, a = 0.f;
    if (M != -INFINITY) {
#pragma unroll
      for (int w = 0; w < AD_WAVES; ++w) {
        const float f = __expf(sm[w][0] - M);
        l += sm[w][1] * f;
        a += sacc[w][tid] * f;
      }
    }
    o[(long)n * hidden + h * D + tid] = l > 0.f ? a / l : 0.f;
  }
}

__global__ __launch_bounds__(256) void kv_append_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                        bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, int N,
                                                        int Lmax, int hidden, int pos) {
  const int hg = hidden / 8;
  const long total = (long)N * hg;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / hg), g = (int)(i % hg);
    const float* src = (blockIdx.y ? v : k) + (long)n * hidden + g * 8;
    bf16_t* dst = (blockIdx.y ? vc : kc) + ((long)n * Lmax + pos) * hidden + g * 8;
    const v4f a = *reinterpret_cast<const v4f*>(src), b = *reinterpret_cast<const v4f*>(src + 4);
    v4u w;
    w[0] = pack2bf(a[0], a[1]);
    w[1] = pack2bf(a[2], a[3]);
    w[2] = pack2bf(b[0], b[1]);
    w[3] = pack2bf(b[2], b[3]);
    *reinterpret_cast<v4u*>(dst) = w;
  }
}

// grid (chunks, N, planes): row n of plane x copies its first len positions (len * hidden / 8 granules of 16 bytes,
// contiguous) from row parent[n] of the same plane of src
__global__ __launch_bounds__(256) void kv_reorder_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                         const int* __restrict__ parent, int N, int Lmax, int hidden,
                                                         int len) {
  const int n = blockIdx.y;
  const long plane = blockIdx.z;
  const int p = min(max(parent[n], 0), N - 1);
  const long row = (long)Lmax * hidden;
  const v4u* s = reinterpret_cast<const v4u*>(src + (plane * N + p) * row);
  v4u* d = reinterpret_cast<v4u*>(dst + (plane * N + n) * row);
  const int gran = len * (hidden / 8);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < gran; i += gridDim.x * blockDim.x) d[i] = s[i];
}

}  // namespace

extern "C" int bigdl_attn_decode(const float* q, const uint16_t* kcache, const uint16_t* vcache, const int* rows,
                                 const float* bias, float* o, int N, int R, int Lmax, int heads, int D, int len,
                                 hipStream_t st) {
  if (N <= 0 || R <= 0 || heads <= 0 || len < 1 || len > Lmax) return -1;
  if (heads > 65535 || (long)Lmax * heads * D > 0x7fffffffL) return -1;
  const int hidden = heads * D;
  const dim3 grid(N, heads), block(AD_THREADS);
#define AD_LAUNCH(DD, GG)                                                                                          \
  hipLaunchKernelGGL((attn_decode_kernel<DD, GG>), grid, block, 0, st, q, kcache, vcache, rows, bias, o, R, Lmax, \
                     hidden, len)
  switch (D) {
    case 32: AD_LAUNCH(32, 4); break;
    case 64: AD_LAUNCH(64, 8); break;
    case 96: AD_LAUNCH(96, 16); break;
    case 128: AD_LAUNCH(128, 16); break;
    default: return -1;
  }
#undef AD_LAUNCH
  HIP_LAUNCH_CHECK();
  return 0;
}

extern "C" int bigdl_kv_append(const float* k, const float* v, uint16_t* kcache, uint16_t* vcache, int N, int Lmax,
                               int hidden, int pos, hipStream_t st) {
  if (N <= 0 || hidden <= 0 || hidden % 8 || pos < 0 || pos >= Lmax) return -1;
  const long total = (long)N * (hidden / 8);
  const dim3 grid((unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256), 2);
  hipLaunchKernelGGL(kv_append_kernel, grid, dim3(256), 0, st, k, v, kcache, vcache, N, Lmax, hidden, pos);
  HIP_LAUNCH_CHECK();
  return 0;
}

extern "C" int bigdl_kv_reorder(const uint16_t* src, uint16_t* dst, const int* parent, int planes, int N, int Lmax,
                                int hidden, int len, hipStream_t st) {
  if (planes <= 0 || planes > 65535 || N <= 0 || N > 65535 || hidden <= 0 || hidden % 8 || len < 1 || len > Lmax)
    return -1;
  if ((long)Lmax * hidden / 8 > 0x7fffffffL || src == dst) return -1;
  const int gran = len * (hidden / 8);
  const int chunks = (gran + 1023) / 1024 > 64 ? 64 : (gran + 1023) / 1024;   // <= 4 granules per thread up to 64 K
  hipLaunchKernelGGL(kv_reorder_kernel, dim3(chunks, N, planes), dim3(256), 0, st, src, dst, parent, N, Lmax, hidden,
                     len);
  HIP_LAUNCH_CHECK();
  return 0;
}
