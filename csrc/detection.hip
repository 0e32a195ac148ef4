// Detection kernels for gfx950: greedy NMS (64-bit IoU masks + single-wave scan), segmented NMS over every
// (image, class) column of a score matrix in one launch (nms_classes_kernel: threshold, sort, top-k cut and greedy
// pass in LDS, one workgroup per segment), segmented top-k in the order of a stable descending sort over segments of
// any length (segmented_topk_flat_kernel / segmented_topk_maps_kernel: radix select, ordered compaction, bitonic sort
// of at most 4096 survivors, one workgroup per segment), RoiAlign forward for one map or for all pyramid levels in
// one launch (roi_align_levels_fwd_kernel; both call roi_align_bin), RoiPooling forward/backward.
//
// Reference semantics: S/nn/Nms.scala:50-236 (greedy NMS over score-sorted boxes, "IoU > thresh" suppresses,
// pixel areas (x2-x1+1)(y2-y1+1) unless normalized), S/nn/RoiAlign.scala:45-420 (bilinear sampling grid,
// out-of-map samples contribute 0 but are counted, average over the grid), S/nn/RoiPooling.scala:42-366
// (Fast R-CNN max pooling over rounded, scaled rois, argmax kept for backward).
//
// NMS mapping: a wave is 64 lanes and a suppression row is a 64-bit word, so block (i, j) of the IoU matrix
// is one wave: lane l tests box j*64+l against box i*64+r for each r and __ballot turns the 64 predicates
// into one word. The greedy pass is then one wave walking the boxes in score order with the "removed" bitset
// held in registers (lane l owns words l, l+64, ...): no barrier, no atomics, and the result never leaves
// the device.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NMS_MAX_WORDS_PER_LANE = 4;   // up to 64 * 64 * 4 = 16384 boxes

__device__ __forceinline__ bool iou_gt(const float* a, const float* b, float area_a, float area_b, float thresh,
                                       float one) {
  const float w = fminf(a[2], b[2]) - fmaxf(a[0], b[0]) + one;
  if (w < 0.f) return false;
  const float h = fminf(a[3], b[3]) - fmaxf(a[1], b[1]) + one;
  if (h < 0.f) return false;
  const float inter = w * h;
  return inter / (area_a + area_b - inter) > thresh;
}

// boxes: [n][4] sorted by descending score. mask: [n][words] uint64, bit l of word j in row i set when box
// j*64+l (j*64+l > i) overlaps box i above thresh.
__global__ void __launch_bounds__(64) nms_mask_kernel(const float* __restrict__ boxes, int n, float thresh,
                                                      int normalized, unsigned long long* __restrict__ mask,
                                                      int words) {
  const int jb = blockIdx.x, ib = blockIdx.y, lane = threadIdx.x;
  const float one = normalized ? 0.f : 1.f;
  __shared__ float col[64][4];
  __shared__ float col_area[64];
  const int j = jb * 64 + lane;
  if (j < n) {
    const float4 b = *reinterpret_cast<const float4*>(boxes + 4 * (size_t)j);
    col[lane][0] = b.x; col[lane][1] = b.y; col[lane][2] = b.z; col[lane][3] = b.w;
    col_area[lane] = (b.z - b.x + one) * (b.w - b.y + one);
  }
  __syncthreads();
  const int rows = min(64, n - ib * 64);
  for (int r = 0; r < rows; ++r) {
    const int i = ib * 64 + r;
    const float4 bi = *reinterpret_cast<const float4*>(boxes + 4 * (size_t)i);   // wave-uniform load
    const float a[4] = {bi.x, bi.y, bi.z, bi.w};
    const float area_i = (bi.z - bi.x + one) * (bi.w - bi.y + one);
    const bool p = (j < n) && (j > i) && iou_gt(a, col[lane], area_i, col_area[lane], thresh, one);
    const unsigned long long word = __ballot(p);
    if (lane == 0) mask[(size_t)i * words + jb] = word;
  }
}

// Single wave: greedy scan in sorted order. keep_out[k] = sorted position of the k-th kept box; count_out[0] = k.
__global__ void __launch_bounds__(64) nms_scan_kernel(const unsigned long long* __restrict__ mask, int n, int words,
                                                      int max_keep, int* __restrict__ keep_out,
                                                      int* __restrict__ count_out) {
  const int lane = threadIdx.x;
  unsigned long long removed[NMS_MAX_WORDS_PER_LANE];
#pragma unroll
  for (int k = 0; k < NMS_MAX_WORDS_PER_LANE; ++k) removed[k] = 0ull;
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    const int w = i >> 6, owner = w & 63, slot = w >> 6;
    unsigned long long mine = 0ull;
#pragma unroll
    for (int k = 0; k < NMS_MAX_WORDS_PER_LANE; ++k)
      if (k == slot) mine = removed[k];
    const unsigned long long ow = __shfl(mine, owner, 64);
    if ((ow >> (i & 63)) & 1ull) continue;          // wave-uniform branch
    if (lane == 0) keep_out[kept] = i;
    ++kept;
    if (max_keep > 0 && kept >= max_keep) break;
    const unsigned long long* row = mask + (size_t)i * words;
#pragma unroll
    for (int k = 0; k < NMS_MAX_WORDS_PER_LANE; ++k) {
      const int wd = lane + 64 * k;
      if (wd < words) removed[k] |= row[wd];
    }
  }
  if (lane == 0) count_out[0] = kept;
}

// ------------------------------------------------------------------------------- segmented (image, class) NMS
// One 256-thread workgroup per (image, class) column slice of scores [R][C]: the rows of image b that pass the
// score test are compacted into LDS in row order (ballot + popcount per wave, wave counts through LDS), sorted by
// (score descending, row ascending) with a bitonic network (the composite compare makes the order total, which is
// the order of a stable descending sort), cut to pre_topk, and walked greedily: when candidate i is alive every
// thread tests its own candidates j > i with iou_gt and clears their alive bytes; a removed candidate is skipped by
// all threads, which read the same byte, so there is one barrier per kept box. Areas sit in LDS for j and in
// registers for i exactly as in nms_mask_kernel, so both kernels evaluate the same expression. No global
// workspace, no atomics, every loop bounded by the candidate count.
constexpr int NMS_MAX_IMAGES = 64;   // row offsets travel by value; the launcher issues one launch per 64 images
struct NmsOffsets { int off[NMS_MAX_IMAGES + 1]; };

template <int CAP>
__global__ void __launch_bounds__(256) nms_classes_kernel(const float* __restrict__ scores,
                                                          const float* __restrict__ boxes,
                                                          unsigned char* __restrict__ keep, int* __restrict__ overflow,
                                                          NmsOffsets offs, int C, int Cb, int skip_class,
                                                          float score_thresh, int inclusive, int pre_topk,
                                                          float nms_thresh, int normalized) {
  __shared__ float key_s[CAP];
  __shared__ int key_r[CAP];
  __shared__ float box[CAP][4];
  __shared__ float box_area[CAP];
  __shared__ unsigned char alive[CAP];
  __shared__ int wave_cnt[4];
  const int b = blockIdx.x / C, c = blockIdx.x % C, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int row0 = offs.off[b], nrows = offs.off[b + 1] - row0;
  for (int r = tid; r < nrows; r += 256) keep[(size_t)(row0 + r) * C + c] = 0;
  if (c == skip_class) return;

  int n = 0;                                            // candidates so far (workgroup-uniform)
  for (int base = 0; base < nrows; base += 256) {
    const int r = base + tid;
    float s = 0.f;
    bool p = false;
    if (r < nrows) {
      s = scores[(size_t)(row0 + r) * C + c];
      p = inclusive ? s >= score_thresh : s > score_thresh;   // NaN fails both
    }
    const unsigned long long m = __ballot(p);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = n + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    if (p && pos < CAP) { key_s[pos] = s; key_r[pos] = r; }
    n += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (n > CAP) {                                        // the caller reruns this call on the per-class path
    if (tid == 0) overflow[0] = 1;
    return;
  }
  if (n == 0) return;

  int P = 2;
  while (P < n) P <<= 1;                                // n <= CAP and CAP is a power of two
  for (int t = n + tid; t < P; t += 256) { key_s[t] = -INFINITY; key_r[t] = 0x7fffffff; }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += 256) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const float sa = key_s[lo], sb = key_s[hi];
        const int ra = key_r[lo], rb = key_r[hi];
        const bool after = sa < sb || (sa == sb && ra > rb);   // a belongs behind b
        if (after == up) {
          key_s[lo] = sb; key_s[hi] = sa;
          key_r[lo] = rb; key_r[hi] = ra;
        }
      }
      __syncthreads();
    }
  }
  if (pre_topk > 0 && n > pre_topk) n = pre_topk;

  const float one = normalized ? 0.f : 1.f;
  const int cb = Cb == 1 ? 0 : c;
  for (int t = tid; t < n; t += 256) {
    const float4 v = *reinterpret_cast<const float4*>(boxes + ((size_t)(row0 + key_r[t]) * Cb + cb) * 4);
    box[t][0] = v.x; box[t][1] = v.y; box[t][2] = v.z; box[t][3] = v.w;
    box_area[t] = (v.z - v.x + one) * (v.w - v.y + one);
    alive[t] = 1;
  }
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    if (!alive[i]) continue;                            // same byte for every thread: uniform
    const float a[4] = {box[i][0], box[i][1], box[i][2], box[i][3]};
    const float area_i = (a[2] - a[0] + one) * (a[3] - a[1] + one);
    int j = (i + 1) - ((i + 1) & 255) + tid;            // first j > i owned by this thread
    if (j <= i) j += 256;
    for (; j < n; j += 256)
      if (alive[j] && iou_gt(a, box[j], area_i, box_area[j], nms_thresh, one)) alive[j] = 0;
    __syncthreads();
  }
  for (int t = tid; t < n; t += 256)
    if (alive[t]) keep[(size_t)(row0 + key_r[t]) * C + c] = 1;
}

// ------------------------------------------------------------------------------------------- segmented top-k
// One 1024-thread workgroup per segment returns the first k elements of the order of a stable descending sort
// (torch.sort(descending=True, stable=True)): NaN first, then larger values, -0.0 == +0.0, ties by lower index.
// topk_sel_key maps a float to a 32-bit key that is larger for an element that comes first and equal exactly for
// elements the order ties. A radix select over the key (four 8-bit digits, an integer histogram in LDS, the segment
// re-read per pass) finds the cut key T and the number of keys above it; one pass in index order then puts every
// key above T into LDS and writes the first k - above elements equal to T straight behind them in the output
// (ballot + popcount ranks, as nms_classes_kernel compacts); a bitonic sort on (key, index) orders the at most
// k - 1 <= 4095 elements above T. No global workspace, integer LDS atomics only, every loop bounded by the segment
// length, and an output slot past the segment's count is filled with index 0 / value 0 without reading anything.
constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int TOPK_UNROLL = 4;         // elements per thread and loop trip
constexpr int TOPK_MAX_K = 4096;
constexpr int TOPK_MAX_SEGMENTS = 64;   // flat mode: offsets travel by value, one launch per 64 segments
struct TopkOffsets { int in[TOPK_MAX_SEGMENTS + 1]; int out[TOPK_MAX_SEGMENTS + 1]; };

__device__ __forceinline__ unsigned topk_sel_key(float v) {
  if (v != v) return 0xffffffffu;                       // every NaN is the same, largest key
  if (v == 0.f) return 0x80000000u;                     // -0.0 and +0.0 tie
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);    // +inf is 0xff800000, -inf 0x007fffff
}

// Flat mode: element i of the segment is values[in0 + i], skipped when mask[in0 + i] == 0.
struct TopkFlatLoader {
  const float* values;
  const unsigned char* mask;
  __device__ __forceinline__ bool load(unsigned i, float& v) const {
    v = values[i];
    return mask == nullptr || mask[i] != 0;
  }
};
// Level-map mode: element i = (h * W + w) * A + a of image n is obj[n][a][h][w].
struct TopkMapLoader {
  const float* obj;    // map of this image: [A][HW]
  int A, HW;
  __device__ __forceinline__ bool load(unsigned i, float& v) const {
    const unsigned hw = i / (unsigned)A, a = i - hw * (unsigned)A;
    v = obj[(size_t)a * HW + hw];
    return true;
  }
};

// The body both modes share. len = segment length, k >= 1; out_idx / out_val point at the segment's first output
// slot and have min(k, len) slots. Returns the number of slots written in rank order (workgroup-uniform); key_s /
// idx_s then hold nothing the caller needs: the ranked indices are in out_idx.
template <class Loader>
__device__ int topk_segment(const Loader& ld, unsigned len, int k, int idx_base, int* out_idx,
                            unsigned* key_s, int* idx_s, int* hist, int* wave_cnt, int* sel) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slots = (int)min((unsigned)k, len);
  // ---- radix select: after pass p the top 8 * (p + 1) bits of T are in `prefix`, `above` counts keys over them
  unsigned prefix = 0;
  int above = 0, want = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int t = tid; t < 256; t += TOPK_THREADS) hist[t] = 0;
    __syncthreads();
    for (unsigned base = 0; base < len; base += TOPK_THREADS * TOPK_UNROLL) {
      bool p[TOPK_UNROLL];
      unsigned key[TOPK_UNROLL];
#pragma unroll
      for (int j = 0; j < TOPK_UNROLL; ++j) {             // the loads of one trip are independent: all in flight
        const unsigned i = base + j * TOPK_THREADS + tid;
        p[j] = false;
        key[j] = 0;
        if (i < len) {
          float v;
          p[j] = ld.load(i, v);
          key[j] = topk_sel_key(v);
          p[j] = p[j] && (pass == 0 || (key[j] >> (shift + 8)) == prefix);
        }
      }
#pragma unroll
      for (int j = 0; j < TOPK_UNROLL; ++j) {
        const unsigned long long m = __ballot(p[j]);
        if (m == 0ull) continue;                          // wave-uniform
        const int digit = (int)((key[j] >> shift) & 0xffu);
        const int d0 = __shfl(digit, __ffsll((long long)m) - 1, 64);
        const unsigned long long same = __ballot(p[j] && digit == d0);
        if (p[j] && digit != d0) atomicAdd(&hist[digit], 1);
        if (lane == 0) atomicAdd(&hist[d0], __popcll(same));   // the common digit of the wave in one add
      }
    }
    __syncthreads();
    if (wave == 0) {                                    // lane l owns digits 255 - 4l .. 252 - 4l, largest first
      int c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = hist[255 - (4 * lane + j)]; s += c[j]; }
      int incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      if (pass == 0) {                                  // the histogram of pass 0 counts every valid element
        const int valid = __shfl(incl, 63, 64);
        if (lane == 0) sel[2] = min(k, valid);
        want = min(k, valid);
      } else {
        want = sel[2];
      }
      int run = above + incl - s;
      if (want > 0 && run < want && want <= run + s) {  // exactly one lane holds the cut
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (run < want && want <= run + c[j]) { sel[0] = 255 - (4 * lane + j); sel[1] = run; }
          run += c[j];
        }
      }
    }
    __syncthreads();
    want = sel[2];
    if (want == 0) break;                               // nothing valid: workgroup-uniform
    prefix = (prefix << 8) | (unsigned)sel[0];
    above = sel[1];
    __syncthreads();                                    // sel and hist are rewritten by the next pass
  }
  if (want == 0) {
    for (int t = tid; t < slots; t += TOPK_THREADS) out_idx[t] = idx_base;
    return 0;
  }
  // ---- compaction in index order: keys above T to LDS slots [0, above), the first want - above keys equal to T
  //      to output slots [above, want)
  const unsigned T = prefix;
  const int need_eq = want - above;
  int n_gt = 0, n_eq = 0;                               // workgroup-uniform running counts
  for (unsigned base = 0; base < len; base += TOPK_THREADS * TOPK_UNROLL) {
    bool gt[TOPK_UNROLL], eq[TOPK_UNROLL];
    unsigned key[TOPK_UNROLL];
    unsigned long long mg[TOPK_UNROLL], me[TOPK_UNROLL];
#pragma unroll
    for (int j = 0; j < TOPK_UNROLL; ++j) {
      const unsigned i = base + j * TOPK_THREADS + tid;
      gt[j] = eq[j] = false;
      key[j] = 0;
      if (i < len) {
        float v;
        const bool p = ld.load(i, v);
        key[j] = topk_sel_key(v);
        gt[j] = p && key[j] > T;
        eq[j] = p && key[j] == T;
      }
    }
#pragma unroll
    for (int j = 0; j < TOPK_UNROLL; ++j) {               // sub-chunk j, wave w: counts at wave_cnt[2 (j W + w)]
      mg[j] = __ballot(gt[j]);
      me[j] = __ballot(eq[j]);
      if (lane == 0) {
        wave_cnt[2 * (j * TOPK_WAVES + wave)] = __popcll(mg[j]);
        wave_cnt[2 * (j * TOPK_WAVES + wave) + 1] = __popcll(me[j]);
      }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < TOPK_UNROLL; ++j) {               // index order: sub-chunk, then wave, then lane
      int pg = n_gt + __popcll(mg[j] & below), pe = n_eq + __popcll(me[j] & below);
      int tg = 0, te = 0;
      for (int w = 0; w < TOPK_WAVES; ++w) {
        const int cg = wave_cnt[2 * (j * TOPK_WAVES + w)], ce = wave_cnt[2 * (j * TOPK_WAVES + w) + 1];
        if (w < wave) { pg += cg; pe += ce; }
        tg += cg; te += ce;
      }
      const int i = (int)(base + j * TOPK_THREADS + tid);
      if (gt[j] && pg < above) { key_s[pg] = key[j]; idx_s[pg] = i; }   // pg < above < k <= TOPK_MAX_K always
      if (eq[j] && pe < need_eq) out_idx[above + pe] = idx_base + i;
      n_gt += tg; n_eq += te;
    }
    __syncthreads();
    if (n_gt >= above && n_eq >= need_eq) break;        // uniform: everything selected has been seen
  }
  // ---- bitonic sort of the keys above T: larger key first, lower index first among equal keys
  int P = 2;
  while (P < above) P <<= 1;                            // above < k <= 4096, so P <= 4096
  for (int t = above + tid; t < P; t += TOPK_THREADS) { key_s[t] = 0u; idx_s[t] = 0x7fffffff; }
  __syncthreads();
  if (above > 1) {
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < P / 2; t += TOPK_THREADS) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const unsigned ka = key_s[lo], kb = key_s[hi];
          const int ia = idx_s[lo], ib = idx_s[hi];
          const bool after = ka < kb || (ka == kb && ia > ib);   // a belongs behind b
          if (after == up) {
            key_s[lo] = kb; key_s[hi] = ka;
            idx_s[lo] = ib; idx_s[hi] = ia;
          }
        }
        __syncthreads();
      }
    }
  }
  for (int t = tid; t < above; t += TOPK_THREADS) out_idx[t] = idx_base + idx_s[t];
  for (int t = want + tid; t < slots; t += TOPK_THREADS) out_idx[t] = idx_base;
  __syncthreads();                                      // out_idx of this segment is read back by the caller
  return want;
}

#define TOPK_SHARED                                                                                               \
  __shared__ unsigned key_s[TOPK_MAX_K];                                                                          \
  __shared__ int idx_s[TOPK_MAX_K];                                                                               \
  __shared__ int hist[256];                                                                                       \
  __shared__ int wave_cnt[2 * TOPK_WAVES * TOPK_UNROLL];                                                          \
  __shared__ int sel[3]

// values [R], mask uint8 [R] or null; segment s of this launch is [offs.in[s], offs.in[s + 1]), its output slots
// start at offs.out[s]. out_idx holds indices within the segment (global_index: into values), counts [S] or null.
__global__ void __launch_bounds__(TOPK_THREADS) segmented_topk_flat_kernel(const float* __restrict__ values,
                                                                            const unsigned char* __restrict__ mask,
                                                                            TopkOffsets offs, int k, int global_index,
                                                                            int* __restrict__ out_idx,
                                                                            float* __restrict__ out_val,
                                                                            int* __restrict__ counts) {
  TOPK_SHARED;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int in0 = offs.in[s];
  const unsigned len = (unsigned)(offs.in[s + 1] - in0);
  if (len == 0) {
    if (counts != nullptr && tid == 0) counts[s] = 0;
    return;
  }
  const TopkFlatLoader ld{values + in0, mask == nullptr ? nullptr : mask + in0};
  int* oi = out_idx + offs.out[s];
  float* ov = out_val + offs.out[s];
  const int base = global_index ? in0 : 0;
  const int n = topk_segment(ld, len, k, base, oi, key_s, idx_s, hist, wave_cnt, sel);
  const int slots = (int)min((unsigned)k, len);
  for (int t = tid; t < slots; t += TOPK_THREADS) ov[t] = t < n ? ld.values[oi[t] - base] : 0.f;
  if (counts != nullptr && tid == 0) counts[s] = n;
}

// Segment (n, l) = blockIdx.x: image n of level l, n-major. Output slots of image n, level l start at
// n * sum_l min(k, HW_l * A) + sum_{l' < l} min(k, HW_l' * A). out_reg / out_anc [slots][4] receive channels
// 4a .. 4a + 3 at (h, w) of reg_l [N][4A][H][W] and row i of the level's anchors [HW * A][4].
__global__ void __launch_bounds__(TOPK_THREADS) segmented_topk_maps_kernel(TopkLevelMaps maps, int k,
                                                                            int* __restrict__ out_idx,
                                                                            float* __restrict__ out_val,
                                                                            float* __restrict__ out_reg,
                                                                            float* __restrict__ out_anc) {
  TOPK_SHARED;
  const int n = blockIdx.x / maps.L, l = blockIdx.x % maps.L, tid = threadIdx.x;
  const int A = maps.A, HW = maps.HW[l];
  int per_image = 0, before = 0;
  for (int j = 0; j < maps.L; ++j) {
    const int sl = (int)min((unsigned)k, (unsigned)maps.HW[j] * (unsigned)A);
    if (j < l) before += sl;
    per_image += sl;
  }
  const size_t out0 = (size_t)n * per_image + before;
  const unsigned len = (unsigned)HW * (unsigned)A;
  const TopkMapLoader ld{maps.obj[l] + (size_t)n * A * HW, A, HW};
  int* oi = out_idx + out0;
  const int cnt = topk_segment(ld, len, k, 0, oi, key_s, idx_s, hist, wave_cnt, sel);   // == min(k, len)
  const float* reg = maps.reg[l] + (size_t)n * 4 * A * HW;
  const float* anc = maps.anc[l];
  for (int t = tid; t < cnt; t += TOPK_THREADS) {
    const unsigned i = (unsigned)oi[t];
    const unsigned hw = i / (unsigned)A, a = i - hw * (unsigned)A;
    float v;
    ld.load(i, v);
    out_val[out0 + t] = v;
    float4 r;
    r.x = reg[(size_t)(4 * a + 0) * HW + hw]; r.y = reg[(size_t)(4 * a + 1) * HW + hw];
    r.z = reg[(size_t)(4 * a + 2) * HW + hw]; r.w = reg[(size_t)(4 * a + 3) * HW + hw];
    reinterpret_cast<float4*>(out_reg)[out0 + t] = r;
    reinterpret_cast<float4*>(out_anc)[out0 + t] = reinterpret_cast<const float4*>(anc)[i];
  }
}
#undef TOPK_SHARED

// ---------------------------------------------------------------------------------------------- RoiAlign
// One output bin (ph, pw) of one roi on one channel plane xc [H][W]; rb = (x1, y1, x2, y2).
__device__ __forceinline__ float roi_align_bin(const float* __restrict__ xc, const float* __restrict__ rb, int H,
                                               int W, int PH, int PW, int ph, int pw, float scale, int sampling) {
  const float sw = rb[0] * scale, sh = rb[1] * scale, ew = rb[2] * scale, eh = rb[3] * scale;
  const float rw = fmaxf(ew - sw, 1.f), rh = fmaxf(eh - sh, 1.f);
  const float bh = rh / PH, bw = rw / PW;
  const int gh = sampling > 0 ? sampling : (int)ceilf(rh / PH);
  const int gw = sampling > 0 ? sampling : (int)ceilf(rw / PW);
  float acc = 0.f;
  for (int iy = 0; iy < gh; ++iy) {
    const float yy = sh + ph * bh + (iy + 0.5f) * bh / gh;
    for (int ix = 0; ix < gw; ++ix) {
      const float xx = sw + pw * bw + (ix + 0.5f) * bw / gw;
      if (yy < -1.f || yy > (float)H || xx < -1.f || xx > (float)W) continue;
      float y = fmaxf(yy, 0.f), xv = fmaxf(xx, 0.f);
      int yl = (int)y, xl = (int)xv, yh, xh;
      if (yl >= H - 1) { yl = yh = H - 1; y = (float)yl; } else { yh = yl + 1; }
      if (xl >= W - 1) { xl = xh = W - 1; xv = (float)xl; } else { xh = xl + 1; }
      const float ly = y - yl, lx = xv - xl, hy = 1.f - ly, hx = 1.f - lx;
      acc += hy * hx * xc[yl * W + xl] + hy * lx * xc[yl * W + xh] + ly * hx * xc[yh * W + xl] +
             ly * lx * xc[yh * W + xh];
    }
  }
  return acc / (float)(gh * gw);
}

// x: [N][C][H][W] fp32; rois: [R][rcols] (rcols 4: batch 0, (x1,y1,x2,y2); rcols 5: (b, x1, y1, x2, y2)).
// One thread per output element (r, c, ph, pw): the sampling grid of one bin is at most a few dozen taps.
__global__ void __launch_bounds__(256) roi_align_fwd_kernel(const float* __restrict__ x, const float* __restrict__ rois,
                                                            float* __restrict__ out, int R, int rcols, int C, int H,
                                                            int W, int PH, int PW, float scale, int sampling) {
  const long total = (long)R * C * PH * PW;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int pw = (int)(idx % PW);
    const int ph = (int)((idx / PW) % PH);
    const int c = (int)((idx / ((long)PW * PH)) % C);
    const int r = (int)(idx / ((long)PW * PH * C));
    const float* roi = rois + (size_t)r * rcols;
    const int b = rcols == 5 ? (int)roi[0] : 0;
    const float* rb = roi + (rcols == 5 ? 1 : 0);
    const float* xc = x + ((size_t)b * C + c) * (size_t)H * W;
    out[idx] = roi_align_bin(xc, rb, H, W, PH, PW, ph, pw, scale, sampling);
  }
}

// All pyramid levels in one launch: roi r samples the map of levels[r]. The level and the batch index are clamped to
// the maps that exist, so a bad index tensor cannot read out of bounds.
__global__ void __launch_bounds__(256) roi_align_levels_fwd_kernel(RoiLevelMaps maps, const float* __restrict__ rois,
                                                                   const int* __restrict__ levels,
                                                                   float* __restrict__ out, int R, int PH, int PW,
                                                                   int sampling) {
  const int C = maps.C;
  const long total = (long)R * C * PH * PW;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int pw = (int)(idx % PW);
    const int ph = (int)((idx / PW) % PH);
    const int c = (int)((idx / ((long)PW * PH)) % C);
    const int r = (int)(idx / ((long)PW * PH * C));
    const float* roi = rois + (size_t)r * 5;
    const int l = min(max(levels[r], 0), maps.L - 1);
    const int b = min(max((int)roi[0], 0), maps.N - 1);
    const int H = maps.H[l], W = maps.W[l];
    const float* xc = maps.x[l] + ((size_t)b * C + c) * (size_t)H * W;
    out[idx] = roi_align_bin(xc, roi + 1, H, W, PH, PW, ph, pw, maps.scale[l], sampling);
  }
}

// --------------------------------------------------------------------------------------------- RoiPooling
__global__ void __launch_bounds__(256) roi_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ rois,
                                                           float* __restrict__ out, int* __restrict__ argmax, int R,
                                                           int C, int H, int W, int PH, int PW, float scale) {
  const long total = (long)R * C * PH * PW;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int pw = (int)(idx % PW);
    const int ph = (int)((idx / PW) % PH);
    const int c = (int)((idx / ((long)PW * PH)) % C);
    const int r = (int)(idx / ((long)PW * PH * C));
    const float* roi = rois + (size_t)r * 5;
    const int b = (int)roi[0];
    const int sw = (int)floorf(roi[1] * scale + 0.5f), sh = (int)floorf(roi[2] * scale + 0.5f);
    const int ew = (int)floorf(roi[3] * scale + 0.5f), eh = (int)floorf(roi[4] * scale + 0.5f);
    const float bh = fmaxf((float)(eh - sh + 1), 1.f) / PH, bw = fmaxf((float)(ew - sw + 1), 1.f) / PW;
    int hs = (int)floorf(ph * bh) + sh, he = (int)ceilf((ph + 1) * bh) + sh;
    int ws = (int)floorf(pw * bw) + sw, we = (int)ceilf((pw + 1) * bw) + sw;
    hs = min(max(hs, 0), H); he = min(max(he, 0), H);
    ws = min(max(ws, 0), W); we = min(max(we, 0), W);
    const float* xc = x + ((size_t)b * C + c) * (size_t)H * W;
    float best = (he <= hs || we <= ws) ? 0.f : -3.402823466e38f;
    int arg = -1;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) {
        const float v = xc[h * W + w];
        if (v > best) { best = v; arg = h * W + w; }
      }
    out[idx] = best;
    argmax[idx] = arg;
  }
}

__global__ void __launch_bounds__(256) roi_pool_bwd_kernel(const float* __restrict__ gy, const int* __restrict__ argmax,
                                                           const float* __restrict__ rois, float* __restrict__ gx,
                                                           int R, int C, int H, int W, int PH, int PW) {
  const long total = (long)R * C * PH * PW;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int a = argmax[idx];
    if (a < 0) continue;
    const int c = (int)((idx / ((long)PW * PH)) % C);
    const int r = (int)(idx / ((long)PW * PH * C));
    const int b = (int)rois[(size_t)r * 5];
    atomicAdd(gx + ((size_t)b * C + c) * (size_t)H * W + a, gy[idx]);
  }
}

int grid_for(long total) { return (int)std::min<long>((total + 255) / 256, 65536); }

}  // namespace

extern "C" {

int bigdl_nms(const float* boxes_sorted, int n, float thresh, int normalized, int max_keep,
              unsigned long long* mask_ws, int* keep_out, int* count_out, hipStream_t st) {
  const int words = (n + 63) / 64;
  if (n <= 0) return bigdl_fill_bytes(count_out, 0, (long)sizeof(int), st), 0;
  if (words > 64 * NMS_MAX_WORDS_PER_LANE) return -1;
  nms_mask_kernel<<<dim3(words, words), 64, 0, st>>>(boxes_sorted, n, thresh, normalized, mask_ws, words);
  nms_scan_kernel<<<1, 64, 0, st>>>(mask_ws, n, words, max_keep, keep_out, count_out);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_roi_align_fwd(const float* x, const float* rois, float* out, int R, int rcols, int C, int H, int W,
                        int PH, int PW, float scale, int sampling, hipStream_t st) {
  const long total = (long)R * C * PH * PW;
  if (total <= 0) return 0;
  roi_align_fwd_kernel<<<grid_for(total), 256, 0, st>>>(x, rois, out, R, rcols, C, H, W, PH, PW, scale, sampling);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_nms_classes(const float* scores, const float* boxes, unsigned char* keep, int* overflow,
                      const int* offsets_host, int B, int C, int Cb, int skip_class, float score_thresh,
                      int inclusive, int pre_topk, float nms_thresh, int normalized, int cap, hipStream_t st) {
  if (B < 0 || C <= 0 || (Cb != 1 && Cb != C)) return -1;
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    if (offsets_host[b + 1] < offsets_host[b]) return -1;
    longest = std::max(longest, offsets_host[b + 1] - offsets_host[b]);
  }
  if (cap == 0) cap = longest <= 256 ? 256 : longest <= 1024 ? 1024 : 4096;
  if (cap != 256 && cap != 1024 && cap != 4096) return -1;
  bigdl_fill_bytes(overflow, 0, (long)sizeof(int), st);
  for (int b0 = 0; b0 < B; b0 += NMS_MAX_IMAGES) {
    const int nb = std::min(NMS_MAX_IMAGES, B - b0);
    if (offsets_host[b0 + nb] == offsets_host[b0]) continue;
    NmsOffsets offs{};
    for (int b = 0; b <= nb; ++b) offs.off[b] = offsets_host[b0 + b];
#define BIGDL_NMS_CLASSES_LAUNCH(CAP)                                                                             \
  nms_classes_kernel<CAP><<<nb * C, 256, 0, st>>>(scores, boxes, keep, overflow, offs, C, Cb, skip_class,        \
                                                  score_thresh, inclusive, pre_topk, nms_thresh, normalized)
    if (cap == 256) BIGDL_NMS_CLASSES_LAUNCH(256);
    else if (cap == 1024) BIGDL_NMS_CLASSES_LAUNCH(1024);
    else BIGDL_NMS_CLASSES_LAUNCH(4096);
#undef BIGDL_NMS_CLASSES_LAUNCH
    HIP_LAUNCH_CHECK();
  }
  return cap;
}

int bigdl_roi_align_levels_fwd(const RoiLevelMaps* maps, const float* rois, const int* levels, float* out, int R,
                               int PH, int PW, int sampling, hipStream_t st) {
  if (maps->L < 1 || maps->L > BIGDL_ROI_MAX_LEVELS || maps->N < 1) return -1;
  const long total = (long)R * maps->C * PH * PW;
  if (total <= 0) return 0;
  roi_align_levels_fwd_kernel<<<grid_for(total), 256, 0, st>>>(*maps, rois, levels, out, R, PH, PW, sampling);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_segmented_topk_flat(const float* values, const unsigned char* mask, const int* in_off_host,
                              const int* out_off_host, int S, int k, int global_index, int* out_idx, float* out_val,
                              int* counts, hipStream_t st) {
  if (S < 0 || k < 1 || k > TOPK_MAX_K) return -1;
  for (int s = 0; s < S; ++s) {
    const long len = (long)in_off_host[s + 1] - in_off_host[s];
    if (len < 0 || in_off_host[s] < 0) return -1;
    if (out_off_host[s + 1] - out_off_host[s] != (int)std::min<long>(k, len)) return -1;
  }
  for (int s0 = 0; s0 < S; s0 += TOPK_MAX_SEGMENTS) {
    const int ns = std::min(TOPK_MAX_SEGMENTS, S - s0);
    TopkOffsets offs{};
    for (int s = 0; s <= ns; ++s) { offs.in[s] = in_off_host[s0 + s]; offs.out[s] = out_off_host[s0 + s]; }
    segmented_topk_flat_kernel<<<ns, TOPK_THREADS, 0, st>>>(values, mask, offs, k, global_index, out_idx, out_val,
                                                            counts == nullptr ? nullptr : counts + s0);
    HIP_LAUNCH_CHECK();
  }
  return 0;
}

int bigdl_segmented_topk_maps(const TopkLevelMaps* maps, int k, int* out_idx, float* out_val, float* out_reg,
                              float* out_anc, hipStream_t st) {
  if (maps->L < 1 || maps->L > BIGDL_ROI_MAX_LEVELS || maps->N < 1 || maps->A < 1 || k < 1 || k > TOPK_MAX_K)
    return -1;
  for (int l = 0; l < maps->L; ++l)
    if (maps->HW[l] < 1 || (long)maps->HW[l] * maps->A >= (1l << 31)) return -1;
  segmented_topk_maps_kernel<<<maps->N * maps->L, TOPK_THREADS, 0, st>>>(*maps, k, out_idx, out_val, out_reg,
                                                                         out_anc);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_roi_pool_fwd(const float* x, const float* rois, float* out, int* argmax, int R, int C, int H, int W,
                       int PH, int PW, float scale, hipStream_t st) {
  const long total = (long)R * C * PH * PW;
  if (total <= 0) return 0;
  roi_pool_fwd_kernel<<<grid_for(total), 256, 0, st>>>(x, rois, out, argmax, R, C, H, W, PH, PW, scale);
  HIP_LAUNCH_CHECK();
  return 0;
}

int bigdl_roi_pool_bwd(const float* gy, const int* argmax, const float* rois, float* gx, int R, int C, int H, int W,
                       int PH, int PW, hipStream_t st) {
  const long total = (long)R * C * PH * PW;
  if (total <= 0) return 0;
  roi_pool_bwd_kernel<<<grid_for(total), 256, 0, st>>>(gy, argmax, rois, gx, R, C, H, W, PH, PW);
  HIP_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
