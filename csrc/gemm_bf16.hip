// Dense bf16 GEMM for gfx950: C = alpha * op(A) * op(B) + bias + beta * C, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16, three operand forms over row-major bf16 operands (inner dimension contiguous):
//   NT  C[M,N] = A[M,K] * B[N,K]^T     both operands K-contiguous              (Linear forward x * W^T)
//   NN  C[M,N] = A[M,K] * B[K,N]       B reduction-strided                     (data gradient gy * W)
//   TN  C[M,N] = A[K,M]^T * B[K,N]     both reduction-strided, K = rows summed (weight gradient gy^T * x)
//
// Tile and pipeline are those of conv_nt_p8_kernel / conv_wgrad_p8_kernel<true> (conv_igemm.hip; the hazard argument
// for the phase structure is in the header comment of conv_nt_p8_kernel) without the tap table and the per-row
// geometry: 256 x 256 outputs per workgroup, BK = 64, 8 waves = 2 M-halves x 4 N-quarters of 128 x 64, two 64 KB LDS
// buffers of four 16 KB pieces filled by LDS-DMA, one piece per phase, counted vmcnt + raw s_barrier, the second
// M-half one barrier behind the first.
//   * a K-contiguous operand is staged as pieces of 128 rows x 128 B, granule g of row r at slot g ^ (r & 7), and
//     read with ds_read_b128 (conv_nt_p8_kernel's layout);
//   * a reduction-strided operand is staged as pieces of 64 reduction rows x 256 B, chunk c of row r at slot
//     c ^ f(r), and read down the rows with ds_read_b64_tr_b16 (conv_wgrad_p8_kernel's layout and slot function).
//   Both swizzles are applied on the DMA source side.
// Every DMA goes through a buffer resource whose num_records is the operand's true byte size: a granule past an
// extent (M / N / K tails, rows of a partial tile) is fetched at an out-of-range offset and lands as zeros, without a
// branch and without touching memory outside the tensor. All inner extents and leading dimensions are multiples of
// 8 elements and the bases 16-byte aligned, so a granule is wholly inside or wholly outside.
//
// Work split: with few tiles the reduction is cut into gridDim.y slices of whole K-tiles. A slice parks its fp32
// accumulators (register order, write-through stores) in its (tile, slice) slot of the workspace, drains them and
// takes a ticket on the tile's counter; the workgroup that draws the last ticket sums every slot in slice order (so
// the result does not depend on arrival order: bitwise reproducible) and runs the epilogue. No second launch, no
// fp32 atomics on C. The tickets follow the slots in the workspace and are zeroed by a fill kernel before the launch.
//
// Epilogue, straight from the accumulators (a lane holds 4 consecutive n of one row m: 16-byte fp32 / 8-byte bf16
// stores): C = alpha * acc + bias[n] + beta * C_old, optional operands read through 0-byte resources when absent,
// tail stores sent to an out-of-range offset. TN only: colsum[m] += colscale * sum_k A[k][m] from MFMAs of the A
// fragments against a ones operand, by the workgroups of tile column 0 alone (slices combined in slice order).
#include "common.h"
#include "kernels.h"
#include "lds_tr.h"     // tr_pair: the transposing reads as inline assembly (no compiler-inserted DMA drain)

namespace {

constexpr int GB_SLOT = 256 * 256 + 256;   // floats per (tile, slice) slot: accumulators + column sums
constexpr int GB_CUS = 256;

__device__ __forceinline__ int gb_f(int r) { return 2 * ((r & 3) | (((r >> 3) & 1) << 2)); }

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, unsigned off, LDS_PTR(void) l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, l, 16, off, 0, 0, 0);
}

template <int FORM>
__global__ __launch_bounds__(512, 2) void gemm_bf16_kernel(GemmBf16Args a) {
  constexpr bool ACOL = FORM == 2, BCOL = FORM != 0;
  constexpr int BKT = 64;
  constexpr int PIECE = 128 * BKT;                 // bf16 elements per piece (16 KB)
  constexpr int BUF = 4 * PIECE;                   // P0 (A q0) P1 (B q0) P2 (A q1) P3 (B q1)
  constexpr int PC = 128;                          // columns of a reduction-strided piece
  __shared__ __attribute__((aligned(1024))) bf16_t lds[2 * BUF + 8];
  int* lastflag = reinterpret_cast<int*>(lds + 2 * BUF);   // in the one LDS array

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int tiles_n = (a.N + 255) / 256, tiles_m = (a.M + 255) / 256;
  const int ntile = tiles_m * tiles_n;
  const int tile = xcd_remap(blockIdx.x, ntile);
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * 256, n0 = tn * 256;
  const int nk_all = (a.K + BKT - 1) / BKT;
  const int slice = blockIdx.y;
  const int kt0 = slice * a.kt_per;
  const int nk = max(0, min(nk_all, kt0 + a.kt_per) - kt0);

  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.a), (short)0, a.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.b), (short)0, a.b_bytes, 0x00020000);
  const unsigned lda2 = a.lda * 2u, ldb2 = a.ldb * 2u;   // row pitches in bytes

  // ---- DMA geometry
  // K-contiguous piece: instruction j of wave w fills piece rows (j * 8 + w) * 8 .. +8 (8 rows x 128 B); lane -> row
  // + (lane >> 3), slot lane & 7, which holds granule (lane & 7) ^ (lane >> 3). Piece row lr of an A piece of
  // quadrant q is tile row (lr >> 6) * 128 + q * 64 + (lr & 63); of a B piece, tile column (lr >> 5) * 64 + q * 32
  // + (lr & 31). Table slot q2 = q * 2 + j.
  // Reduction-strided piece: instruction j of wave w fills piece rows (j * 8 + w) * 4 .. +4 (4 rows x 256 B); lane ->
  // row + (lane >> 4), slot lane & 15, which holds chunk (lane & 15) ^ f(row), f constant per lane and wave. Piece
  // column pc of an A piece is tile row (pc >> 6) * 128 + q * 64 + (pc & 63); of a B piece, tile column
  // (pc >> 5) * 64 + q * 32 + (pc & 31). Table slot q.
  const int gsrc = (lane & 7) ^ (lane >> 3);
  const int chunk = (lane & 15) ^ gb_f((lane >> 4) | (((wave >> 1) & 1) << 3));
  unsigned aoff[4], boff[4];
  bool aval[4], bval[4];
#pragma unroll
  for (int q2 = 0; q2 < 4; ++q2) {
    const int q = q2 >> 1, lr = ((q2 & 1) * 8 + wave) * 8 + (lane >> 3);
    if (ACOL) {
      const int pc = chunk * 8;
      const int m = m0 + (pc >> 6) * 128 + (q2 & 1) * 64 + (pc & 63);   // slot q2 & 1 = quadrant
      aval[q2] = m < a.M;
      aoff[q2] = (unsigned)m * 2u;
    } else {
      const int m = m0 + (lr >> 6) * 128 + q * 64 + (lr & 63);
      aval[q2] = m < a.M;
      aoff[q2] = (unsigned)m * lda2 + gsrc * 16u;
    }
    if (BCOL) {
      const int pc = chunk * 8;
      const int n = n0 + (pc >> 5) * 64 + (q2 & 1) * 32 + (pc & 31);
      bval[q2] = n < a.N;
      boff[q2] = (unsigned)n * 2u;
    } else {
      const int n = n0 + (lr >> 5) * 64 + q * 32 + (lr & 31);
      bval[q2] = n < a.N;
      boff[q2] = (unsigned)n * ldb2 + gsrc * 16u;
    }
  }
  // piece P of K-tile kt into buffer buf: 2 DMA instructions per thread, invalid granules at the out-of-range offset
  auto issue = [&](int kt, int buf, int P) {
    bf16_t* base = lds + buf * BUF + P * PIECE;
    const int q = P >> 1;
    const int k0 = kt * BKT;
    const bool isA = (P & 1) == 0;
    if (isA ? ACOL : BCOL) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = k0 + (j * 8 + wave) * 4 + (lane >> 4);
        const bool ok = k < a.K && (isA ? aval[q] : bval[q]);
        const unsigned off = isA ? (unsigned)k * lda2 + aoff[q] : (unsigned)k * ldb2 + boff[q];
        dma16(isA ? ra : rb, ok ? off : (isA ? a.a_bytes : a.b_bytes), (LDS_PTR(void))(base + (j * 8 + wave) * 4 * PC));
      }
    } else {
      const bool kin = k0 + gsrc * 8 < a.K;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int q2 = q * 2 + j;
        const bool ok = kin && (isA ? aval[q2] : bval[q2]);
        const unsigned off = (isA ? aoff[q2] : boff[q2]) + (unsigned)k0 * 2u;
        dma16(isA ? ra : rb, ok ? off : (isA ? a.a_bytes : a.b_bytes), (LDS_PTR(void))(base + (j * 8 + wave) * 8 * BKT));
      }
    }
  };

  // ---- fragment reads
  // K-contiguous: granule kh * 4 + (lane >> 4) of piece row (lane & 15) + 16 i lives at slot ^ (lane & 7)
  const int fo0 = (lane & 15) * BKT + (((lane >> 4)) ^ (lane & 7)) * 8;
  const int fo1 = (lane & 15) * BKT + ((4 + (lane >> 4)) ^ (lane & 7)) * 8;
  // reduction-strided: lane 4q'+p of 16-lane group g supplies row 32 kh + 8 g + q' (+4), columns c0 + 4p
  const int G = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  // (f is the same for rows r, r + 4 and r + 32: the K-half and the second row are immediate offsets of 8192 and
  // 1024 bytes from the lane's byte offset of row 8 g + q')
  auto tr_off = [&](int c0) -> unsigned {
    const int row = 8 * G + qq, col = c0 + 4 * pp;
    return (unsigned)(row * PC + (((col >> 3) ^ gb_f(row)) << 3) + (col & 7)) * 2u;
  };
  unsigned atr[4], btr[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) atr[i] = tr_off(wm * 64 + i * 16);
#pragma unroll
  for (int j = 0; j < 2; ++j) btr[j] = tr_off(wn * 32 + j * 16);
  auto lds_addr = [&](const bf16_t* P) -> unsigned {
    return (unsigned)(uintptr_t)(LDS_PTR(const bf16_t))(P);
  };

  v4f acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
  // fragments as two 8-byte halves [.., K-half, lo / hi]: the transposing reads fill a half each, and the halves are
  // joined only behind the s_waitcnt lgkmcnt(0) of the COMPUTE segment
  v4s fa[4][2][2], fb[4][2][2];
  auto split = [&](const v8s v, v4s* d) {
    d[0] = v4s{v[0], v[1], v[2], v[3]};
    d[1] = v4s{v[4], v[5], v[6], v[7]};
  };
  auto join = [&](const v4s* d) -> v8s { return v8s{d[0][0], d[0][1], d[0][2], d[0][3], d[1][0], d[1][1], d[1][2], d[1][3]}; };
  auto read_a = [&](const bf16_t* P) {
    const unsigned pa = lds_addr(P);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ACOL) {
        tr_pair<0>(pa + atr[i], fa[i][0][0], fa[i][0][1]);
        tr_pair<8192>(pa + atr[i], fa[i][1][0], fa[i][1][1]);
      } else {
        split(*reinterpret_cast<const v8s*>(P + (wm * 64 + i * 16) * BKT + fo0), fa[i][0]);
        split(*reinterpret_cast<const v8s*>(P + (wm * 64 + i * 16) * BKT + fo1), fa[i][1]);
      }
    }
  };
  auto read_b = [&](const bf16_t* P, int jb) {
    const unsigned pb = lds_addr(P);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (BCOL) {
        tr_pair<0>(pb + btr[j], fb[jb + j][0][0], fb[jb + j][0][1]);
        tr_pair<8192>(pb + btr[j], fb[jb + j][1][0], fb[jb + j][1][1]);
      } else {
        split(*reinterpret_cast<const v8s*>(P + (wn * 32 + j * 16) * BKT + fo0), fb[jb + j][0]);
        split(*reinterpret_cast<const v8s*>(P + (wn * 32 + j * 16) * BKT + fo1), fb[jb + j][1]);
      }
    }
  };
  // 16 MFMAs of one 64 x 32 quadrant, K-halves outermost; D rows = n, columns = m
  auto quad = [&](int ib, int jb) {
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[ib + i][jb + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(join(fb[jb + j][kh]), join(fa[i][kh]), acc[ib + i][jb + j], 0, 0, 0);
  };
  // column sums (TN, tile column 0): wave wn sums A fragment i = wn of each quadrant against ones, so the four
  // N-quarter waves of an M-half cover its 8 fragments with 4 extra MFMAs per K-tile each
  const bool do_cs = ACOL && a.colsum != nullptr && tn == 0;
  v4f cs[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
  auto colsum = [&](int h) {
    const short one = 0x3f80;
    const v8s ones = {one, one, one, one, one, one, one, one};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (wn == i) {
        cs[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, join(fa[i][0]), cs[h], 0, 0, 0);
        cs[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, join(fa[i][1]), cs[h], 0, 0, 0);
      }
  };
  auto compute = [&](int ib, int jb, int csh) {
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    quad(ib, jb);
    if (ACOL && csh >= 0 && do_cs) colsum(csh);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
  };

  // prologue: K-tile 0 whole, then P0, P1 of K-tile 1; retire P0, P1 of K-tile 0
  if (nk > 0) {
    issue(kt0, 0, 0); issue(kt0, 0, 1); issue(kt0, 0, 3); issue(kt0, 0, 2);
  }
  if (nk > 1) {
    issue(kt0 + 1, 1, 0); issue(kt0 + 1, 1, 1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();     // stagger: the second M-half runs one barrier behind

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bf16_t* L = lds + cur * BUF;
    const bool n1 = kt + 1 < nk, n2 = kt + 2 < nk;
    // ---- phase 0
    if (n1) issue(kt0 + kt + 1, cur ^ 1, 3);
    read_a(L); read_b(L + PIECE, 0);
    if (n1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");          // P3(t) landed
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    compute(0, 0, 0);
    // ---- phase 1
    if (n1) issue(kt0 + kt + 1, cur ^ 1, 2);
    read_b(L + 3 * PIECE, 2);
    if (n1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");          // P2(t) landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    compute(0, 2, -1);
    // ---- phase 2
    if (n2) issue(kt0 + kt + 2, cur, 0);
    read_a(L + 2 * PIECE);
    compute(4, 2, 1);
    // ---- phase 3
    if (n2) issue(kt0 + kt + 2, cur, 1);
    if (n2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");          // P0, P1(t+1) landed
    else if (n1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    compute(4, 0, -1);
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();     // balance the stagger: every wave has left the K-loop
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- split reduction: park, ticket, last arriver sums in slice order
  const int nslice = gridDim.y;
  if (nslice > 1) {
    float* slots = a.ws + (size_t)tile * nslice * GB_SLOT;
    {
      const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(slots + (size_t)slice * GB_SLOT, (short)0,
                                                                         GB_SLOT * 4, 0x00020000);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, acc[i][j]), r, (((i * 4 + j) * 512 + tid) * 4) * 4,
                                                 0, 16);   // sc1: write-through
      if (do_cs && lane < 16) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, cs[h][0]), r,
                                                (65536 + wm * 128 + (4 * h + wn) * 16 + lane) * 4, 0, 16);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its slot stores have left
    __syncthreads();
    if (tid == 0) {
      unsigned* cnt = reinterpret_cast<unsigned*>(a.ws + (size_t)ntile * nslice * GB_SLOT) + tile;
      const unsigned prev = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *lastflag = (prev == (unsigned)(nslice - 1)) ? 1 : 0;
    }
    __syncthreads();
    if (*lastflag == 0) return;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    cs[0] = cs[1] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nslice; ++s) {
      const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(slots + (size_t)s * GB_SLOT, (short)0,
                                                                         GB_SLOT * 4, 0x00020000);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i & 1) asm volatile("" ::: "memory");     // <= 8 slot loads in flight (VGPR budget)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] += __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, (((i * 4 + j) * 512 + tid) * 4) * 4, 0, 16));
      }
      if (do_cs) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          cs[h][0] += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                          r, (65536 + wm * 128 + (4 * h + wn) * 16 + (lane & 15)) * 4, 0, 16));
      }
    }
  }

  // ---- epilogue. acc[i][j][e] = C[m0 + wm * 128 + 16 i + (lane & 15)][n0 + wn * 64 + 16 j + 4 (lane >> 4) + e]
  if (do_cs && lane < 16) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = m0 + wm * 128 + (4 * h + wn) * 16 + lane;
      if (m < a.M) a.colsum[m] += a.colscale * cs[h][0];
    }
  }
  const unsigned esz = a.out_bf16 ? 2u : 4u;
  const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(a.c, (short)0, a.c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rcold = __builtin_amdgcn_make_buffer_rsrc(a.c, (short)0, a.beta != 0.f ? a.c_bytes : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb32 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(a.bias), (short)0, (a.bias && !a.bias_bf16) ? (unsigned)a.N * 4u : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb16 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(a.bias), (short)0, (a.bias && a.bias_bf16) ? (unsigned)a.N * 2u : 0u, 0x00020000);
  const unsigned ldcb = (unsigned)a.ldc * esz;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
    const bool nok = n < a.N;                      // N % 8 == 0: the four columns are in or out together
    v4f bv = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rb32, (unsigned)n * 4u, 0, 0));
    const v2u b16 = __builtin_amdgcn_raw_buffer_load_b64(rb16, (unsigned)n * 2u, 0, 0);
    bv += v4f{lo_bf(b16[0]), hi_bf(b16[0]), lo_bf(b16[1]), hi_bf(b16[1])};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + wm * 128 + i * 16 + (lane & 15);
      const unsigned off = (nok && m < a.M) ? (unsigned)m * ldcb + (unsigned)n * esz : a.c_bytes;
      v4f v = a.alpha * acc[i][j] + bv;
      if (a.out_bf16) {
        __builtin_amdgcn_raw_buffer_store_b64(v2u{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])}, rc, off, 0, 0);
      } else {
        const v4f old = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rcold, off, 0, 0));
        v += a.beta * old;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), rc, off, 0, 0);
      }
    }
  }
}

// slices of whole K-tiles: aim at one workgroup per CU, at least 8 K-tiles per slice, at most 16 slices
void gb_split(int M, int N, int K, int* nslice, int* kt_per) {
  const long tiles = (long)((M + 255) / 256) * ((N + 255) / 256);
  const int nk = (K + 63) / 64;
  long s = GB_CUS / tiles;
  if (s > nk / 8) s = nk / 8;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  const int per = (int)((nk + s - 1) / s);
  *kt_per = per < 1 ? 1 : per;
  *nslice = nk > 0 ? (nk + *kt_per - 1) / *kt_per : 1;
}

}  // namespace

extern "C" size_t bigdl_gemm_bf16_ws_bytes(int form, int M, int N, int K) {
  (void)form;
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int ns, per;
  gb_split(M, N, K, &ns, &per);
  if (ns <= 1) return 0;
  const size_t tiles = (size_t)((M + 255) / 256) * ((N + 255) / 256);
  return tiles * ns * GB_SLOT * sizeof(float) + tiles * sizeof(unsigned);
}

// 0 ok; -1 bad form / extents / alignment; -2 an operand's byte extent does not fit the 32-bit buffer offset;
// -3 workspace missing or too small; -4 beta with bf16 output, bias / colsum with the wrong form
extern "C" int bigdl_gemm_bf16(const GemmBf16Args* in, size_t ws_bytes, hipStream_t st) {
  GemmBf16Args a = *in;
  if (a.form < 0 || a.form > 2 || a.M <= 0 || a.N <= 0 || a.K <= 0) return -1;
  const bool acol = a.form == 2, bcol = a.form != 0;
  const long a_rows = acol ? a.K : a.M, a_in = acol ? a.M : a.K;
  const long b_rows = bcol ? a.K : a.N, b_in = bcol ? a.N : a.K;
  if (a_in % 8 || b_in % 8 || a.N % 8 || a.lda % 8 || a.ldb % 8 || a.ldc % 8) return -1;
  if (a.lda < a_in || a.ldb < b_in || a.ldc < a.N) return -1;
  if (((uintptr_t)a.a | (uintptr_t)a.b | (uintptr_t)a.c | (uintptr_t)a.bias) & 15) return -1;
  if (a.out_bf16 && a.beta != 0.f) return -4;
  if ((a.bias && acol) || (a.colsum && !acol)) return -4;
  const unsigned long long lim = 0xffffff00ull;      // offsets and the out-of-range offset stay below 2^32
  const unsigned long long ab = ((unsigned long long)(a_rows - 1) * a.lda + a_in) * 2ull;
  const unsigned long long bb = ((unsigned long long)(b_rows - 1) * a.ldb + b_in) * 2ull;
  const unsigned long long cb = ((unsigned long long)(a.M - 1) * a.ldc + a.N) * (a.out_bf16 ? 2ull : 4ull);
  // a granule of a tile row past the extent is never addressed (it goes to the out-of-range offset), but its offset
  // is computed in 32 bits first: the full pitch of one tile past the last row must not wrap either
  const unsigned long long apad = ((unsigned long long)(a_rows + 320) * a.lda) * 2ull;
  const unsigned long long bpad = ((unsigned long long)(b_rows + 320) * a.ldb) * 2ull;
  const unsigned long long cpad = ((unsigned long long)(a.M + 320) * a.ldc) * 4ull;
  if (ab > lim || bb > lim || cb > lim || apad > lim || bpad > lim || cpad > lim) return -2;
  a.a_bytes = (unsigned)ab; a.b_bytes = (unsigned)bb; a.c_bytes = (unsigned)cb;
  int ns, per;
  gb_split(a.M, a.N, a.K, &ns, &per);
  a.kt_per = per;
  const int tiles = ((a.M + 255) / 256) * ((a.N + 255) / 256);
  if (ns > 1) {
    if (!a.ws || ws_bytes < bigdl_gemm_bf16_ws_bytes(a.form, a.M, a.N, a.K)) return -3;
    unsigned* tickets = reinterpret_cast<unsigned*>(a.ws + (size_t)tiles * ns * GB_SLOT);
    bigdl_fill_bytes(tickets, 0, (long)tiles * sizeof(unsigned), st);   // a kernel: graph-safe
  }
  dim3 grid(tiles, ns);
  if (a.form == 0) gemm_bf16_kernel<0><<<grid, 512, 0, st>>>(a);
  else if (a.form == 1) gemm_bf16_kernel<1><<<grid, 512, 0, st>>>(a);
  else gemm_bf16_kernel<2><<<grid, 512, 0, st>>>(a);
  HIP_LAUNCH_CHECK();
  return 0;
}
