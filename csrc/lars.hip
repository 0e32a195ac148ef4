// Fused LARS for gfx950: the sums of squares of every layer and the update of every layer in three launches.
//
// Reference: S/optim/LarsSGD.scala:47 (one LarsSGD per layer, a dozen element-wise tensor ops each) and its
// LarsProcessor (LarsSGD.scala:288-340: per-layer ||w||^2 and ||g||^2 reduced over the partitions). Here the layers
// of the flat fp32 master buffer are described by tables (kernels.h): a piece is [lo, hi) of one layer, a chunk is up
// to BIGDL_LARS_CHUNK consecutive elements of one piece, and one 256-thread workgroup works on one chunk at a time
// (grid-strided over the chunks above BIGDL_LARS_BLOCK_CAP blocks).
//
//   lars_norms_kernel         chunk c -> ws[2 c], ws[2 c + 1] = sum w^2, sum g^2 (plain stores)
//   lars_norms_finish_kernel  one wave per layer: lane l adds the layer's chunk partials l, l + 64, ... in ascending
//                             order, then the fixed shuffle tree; acc[2 layer], acc[2 layer + 1] are stored
//   lars_update_kernel        scale and rate once per workgroup, then v = momentum v + (g + wd w) rate, w -= v,
//                             w16 = bf16(w)
//
// No atomics, no zero fill and no waits between workgroups: every partial has one writer and the order of every sum
// is fixed by the tables, so the sums are bitwise reproducible in every mode.
//
// A chunk starts at any element: the elements up to the next 16-byte boundary (the head, at most 3) and those after
// the last whole group of four (the tail) go one per lane, the rest as 16-byte accesses, a lane taking the groups
// tid, tid + 256, ... (4 at most). The body loads are unconditional: a lane past the end of a short chunk re-reads
// the chunk's last group and its values are dropped by a select, so every load is issued before the first wait.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int CH = BIGDL_LARS_CHUNK;
constexpr int PER = CH / (256 * 4);       // 16-byte groups per lane of a full chunk
static_assert(PER * 256 * 4 == CH, "a chunk is a whole number of 16-byte groups per lane");

struct Span {
  long s;        // first element
  long b;        // first element of the 16-byte body
  int h, nb, t;  // head elements, body groups, tail elements
};

// the split of chunk [s, s + n) for buffers whose element 0 sits `phase` elements past a 16-byte boundary
__device__ __forceinline__ Span span_of(long s, long hi, int phase) {
  Span q;
  const long left = hi - s;
  const int n = left < CH ? (int)left : CH;
  int h = (4 - (int)((s + phase) & 3)) & 3;
  if (h > n) h = n;
  q.s = s; q.h = h; q.b = s + h;
  q.nb = (n - h) >> 2;
  q.t = n - h - (q.nb << 2);
  return q;
}

__device__ __forceinline__ int phase_of(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

__global__ __launch_bounds__(256) void lars_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                         const int* __restrict__ chunk_piece,
                                                         const long* __restrict__ chunk_start,
                                                         const long* __restrict__ piece_tab, float* __restrict__ ws,
                                                         int nchunks) {
  __shared__ float part[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int phase = phase_of(w);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Span q = span_of(chunk_start[c], piece_tab[4 * (long)chunk_piece[c] + 1], phase);
    float aw = 0.f, ag = 0.f;
    if (tid < q.h) {
      const float x = w[q.s + tid], y = g[q.s + tid];
      aw += x * x; ag += y * y;
    }
    if (q.nb > 0) {
      const v4f* wb = reinterpret_cast<const v4f*>(w + q.b);
      const v4f* gb = reinterpret_cast<const v4f*>(g + q.b);
      v4f x[PER], y[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int j = tid + 256 * u;
        x[u] = wb[j < q.nb ? j : q.nb - 1];
        y[u] = gb[j < q.nb ? j : q.nb - 1];
      }
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const bool in = tid + 256 * u < q.nb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xe = in ? x[u][e] : 0.f, ye = in ? y[u][e] : 0.f;
          aw += xe * xe; ag += ye * ye;
        }
      }
    }
    if (tid < q.t) {
      const long i = q.b + 4 * (long)q.nb + tid;
      const float x = w[i], y = g[i];
      aw += x * x; ag += y * y;
    }
    aw = wave_sum(aw);
    ag = wave_sum(ag);
    if (lane == 0) { part[0][wave] = aw; part[1][wave] = ag; }
    __syncthreads();
    if (tid == 0) {
      ws[2 * (long)c] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
      ws[2 * (long)c + 1] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void lars_norms_finish_kernel(const float* __restrict__ ws,
                                                               const int* __restrict__ layer_chunks,
                                                               float* __restrict__ acc) {
  const int layer = blockIdx.x, lane = threadIdx.x;
  const int first = layer_chunks[2 * layer], end = layer_chunks[2 * layer + 1];
  float aw = 0.f, ag = 0.f;
  for (int c = first + lane; c < end; c += 64) {
    aw += ws[2 * (long)c];
    ag += ws[2 * (long)c + 1];
  }
  aw = wave_sum(aw);
  ag = wave_sum(ag);
  if (lane == 0) { acc[2 * layer] = aw; acc[2 * layer + 1] = ag; }
}

// the layer's gradient scale with the reference's guards (LarsSGD.scala getGradientScale), in the order the torch
// route applies them: inf -> 1e4, |scale| < 1e-4 -> 1e-4, nan -> 1. The roots and the division run in fp64 and are
// rounded once; this runs once per workgroup.
__device__ __forceinline__ float lars_scale(float sum_w, float sum_g, double WD) {
  const double nw = sqrt((double)sum_w), ng = sqrt((double)sum_g);
  float s = (float)((ng + WD * nw) / nw);
  if (isinf(s)) s = 1e4f;
  if (fabsf(s) < 1e-4f) s = 1e-4f;
  if (isnan(s)) s = 1.f;
  return s;
}

__device__ __forceinline__ void lars_one(float& w, float g, float& v, float wd, float mom, float rate) {
  v = mom * v + (g + wd * w) * rate;
  w -= v;
}

__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ v, bf16_t* __restrict__ w16,
                                                          const int* __restrict__ chunk_piece,
                                                          const long* __restrict__ chunk_start,
                                                          const long* __restrict__ piece_tab,
                                                          const float* __restrict__ piece_hp,
                                                          const float* __restrict__ rates,
                                                          const float* __restrict__ acc, double WD, int nchunks) {
  const int tid = threadIdx.x;
  const int phase = phase_of(w);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long p = chunk_piece[c];
    const long hi = piece_tab[4 * p + 1], dv = piece_tab[4 * p + 2], layer = piece_tab[4 * p + 3];
    const float wd = piece_hp[2 * p], mom = piece_hp[2 * p + 1];
    const float rate = rates[p] / lars_scale(acc[2 * layer], acc[2 * layer + 1], WD);
    const Span q = span_of(chunk_start[c], hi, phase);
    if (tid < q.h) {
      const long i = q.s + tid;
      float x = w[i], m = v[i + dv];
      lars_one(x, g[i], m, wd, mom, rate);
      w[i] = x; v[i + dv] = m;
      if (w16) w16[i] = f2bf(x);
    }
    if (q.nb > 0) {
      v4f* wb = reinterpret_cast<v4f*>(w + q.b);
      const v4f* gb = reinterpret_cast<const v4f*>(g + q.b);
      v4f* vb = reinterpret_cast<v4f*>(v + q.b + dv);
      v4f x[PER], y[PER], m[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int j = tid + 256 * u, jj = j < q.nb ? j : q.nb - 1;
        x[u] = wb[jj];
        y[u] = gb[jj];
        m[u] = vb[jj];
      }
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int j = tid + 256 * u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float xe = x[u][e], me = m[u][e];
          lars_one(xe, y[u][e], me, wd, mom, rate);
          x[u][e] = xe; m[u][e] = me;
        }
        if (j < q.nb) {
          wb[j] = x[u];
          vb[j] = m[u];
          if (w16)
            reinterpret_cast<v2u*>(w16 + q.b)[j] = v2u{pack2bf(x[u][0], x[u][1]), pack2bf(x[u][2], x[u][3])};
        }
      }
    }
    if (tid < q.t) {
      const long i = q.b + 4 * (long)q.nb + tid;
      float x = w[i], m = v[i + dv];
      lars_one(x, g[i], m, wd, mom, rate);
      w[i] = x; v[i + dv] = m;
      if (w16) w16[i] = f2bf(x);
    }
  }
}

inline int lars_grid(int nchunks) { return nchunks < BIGDL_LARS_BLOCK_CAP ? nchunks : BIGDL_LARS_BLOCK_CAP; }

}  // namespace

extern "C" {

int bigdl_lars_norms(const float* w, const float* g, const int* chunk_piece, const long* chunk_start,
                     const long* piece_tab, const int* layer_chunks, float* ws, float* acc, int nchunks, int nlayers,
                     hipStream_t st) {
  if (nchunks < 0 || nlayers < 0) return -1;
  if (((reinterpret_cast<uintptr_t>(w) ^ reinterpret_cast<uintptr_t>(g)) & 15) != 0) return -1;
  if (nchunks > 0)
    lars_norms_kernel<<<lars_grid(nchunks), 256, 0, st>>>(w, g, chunk_piece, chunk_start, piece_tab, ws, nchunks);
  if (nlayers > 0) lars_norms_finish_kernel<<<nlayers, 64, 0, st>>>(ws, layer_chunks, acc);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_lars_update(float* w, const float* g, float* v, uint16_t* w16, const int* chunk_piece,
                      const long* chunk_start, const long* piece_tab, const float* piece_hp, const float* rates,
                      const float* acc, double WD, int nchunks, hipStream_t st) {
  if (nchunks < 0) return -1;
  const uintptr_t a = reinterpret_cast<uintptr_t>(w);
  if (((a ^ reinterpret_cast<uintptr_t>(g)) & 15) != 0 || ((a ^ reinterpret_cast<uintptr_t>(v)) & 15) != 0) return -1;
  // bf16 element i sits at half the byte offset: the same phase means (w16 address / 2) == (w address / 4) mod 4
  if (w16 && (((reinterpret_cast<uintptr_t>(w16) >> 1) ^ (a >> 2)) & 3) != 0) return -1;
  if (nchunks > 0)
    lars_update_kernel<<<lars_grid(nchunks), 256, 0, st>>>(w, g, v, w16, chunk_piece, chunk_start, piece_tab,
                                                           piece_hp, rates, acc, WD, nchunks);
  HIP_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
