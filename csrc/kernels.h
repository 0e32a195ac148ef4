// C ABI of the bigdl_amd HIP kernel library (csrc/*.hip). The torch binding layer
// (csrc/bindings.cpp) is the only caller; the kernels themselves never include torch headers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CONV_MAX_TAPS 64
// Implicit-GEMM "NT" convolution launch (forward, or one stride phase of the data gradient):
//   out[orow(m)][n] = sum_{t < ntaps, c < Cs} src[pix(m) + (o_h*mul_h + tap_h[t], o_w*mul_w + tap_w[t])][c]
//                                             * wt[n*ldw + tap_k[t]*Cs + c]
// where m = (nb, o_h, o_w) over the Nb x OH x OW grid and orow(m) places the row in an OHo x OWo output grid
// at (o_h*omul_h + ooff_h, o_w*omul_w + ooff_w) (identity when ident_out).
struct ConvArgs {
  const uint16_t* src;
  const uint16_t* wt;
  uint16_t* out;
  const float* bias;
  float* stats;
  const uint16_t* addend;   // optional [rows][ldo] bf16 added in the epilogue (same placement as out)
  const uint8_t* addzm;     // optional sign mask of the addend ([rows][Ncol / 8] bytes, ldo == Ncol): the addend is
                            // added only where its bit is set (a ResNet block's residual gradient dz * (y > 0))
  // Optional BN-backward reduction of the consumer BatchNorm (data-gradient GEMMs only): with bnred set the
  // epilogue accumulates sum(dm) and sum(dm * (x - mean)) per channel into [STAT_SLOTS][2][Ncol] slots, where
  // dm = out masked by the fused ReLU (z > 0 when bnz is set, else x * aff[c] + aff[Ncol + c] > 0, else no mask)
  const uint16_t* bnx;      // BN input x, same placement / ldo as out
  const uint16_t* bnz;      // BN output (post residual + ReLU) or nullptr
  const uint8_t* bnzm;      // or its sign mask ([rows][Ncol / 8] bytes, bigdl_bn_apply zm), same placement / ldo
  const float* bnmean;      // [Ncol] batch mean
  const float* bnaff;       // [2 Ncol] scale | shift or nullptr
  float* bnred;
  int Nb, Hs, Ws, Cs;
  int OH, OW;
  int mul_h, mul_w;
  int ntaps, ldw;
  int M, Ncol, Kdim, ldo;
  int OHo, OWo, omul_h, omul_w, ooff_h, ooff_w, ident_out;
  int relu;
  short tap_h[CONV_MAX_TAPS], tap_w[CONV_MAX_TAPS], tap_k[CONV_MAX_TAPS];
  // fp32 output instead of bf16 (same placement / ldo), += into it when accum32: weight gradients of GEMM-shaped
  // layers computed as an NT GEMM over transposed operands (LDS-transposed epilogue only; no stats / bn / relu)
  float* out32;
  int accum32;
  // split-K (256 x 256 kernel on grids that do not fill the chip): fp32 partials [ksplit][M][Ncol] in ws, summed
  // by the split-K epilogue kernel, which applies everything the fused epilogue would. The caller allocates ws
  // (ConvChoice::ws_floats); bigdl_conv_nt fills ksplit from the choice
  float* ws;
  int ksplit;
  // elements between consecutive source pixels (0 = Cs). pstride < Cs views a row of small pixels as overlapping
  // windows of Cs elements: the bf16 stem's pixel pairs (stem.hip) read 4 consecutive pairs (all 7 width taps of
  // one output column) as one 32-element "pixel" (conv_nt_g4_kernel only)
  int pstride;
  // optional [2 Cs] fp32 scale | shift of a training BatchNorm + ReLU that produced the source: the kernel reads
  // relu(x * scale[c] + shift[c]) (rounded to bf16, bit-equal to bigdl_bn_apply's output) instead of x, and zero
  // padding stays zero — the BN output is never materialised (forward GEMMs of the streaming 1x1 and halo 3x3
  // kernels only: any other choice is refused, CONV_ERR_PRE)
  const float* pre;
  // Subsampled ("compact") addend: with add_sh > 1 the addend is an [Nb][add_H][add_W][ldo] tensor at 1 / (add_sh,
  // add_sw) of the output resolution (the data gradient of a 1x1 / stride-s projection shortcut, kept at its own
  // output resolution) and output pixel (n, h, w) adds addend[n][h / add_sh][w / add_sw] when h % add_sh == 0 and
  // w % add_sw == 0, else nothing. add_sh <= 1: the addend has the output's placement. Identity output rows only;
  // add_m* are the multiply-high reciprocals of OW, OH, add_sh, add_sw (bigdl_conv_addend_stride fills them; the
  // streaming 1x1 EXT epilogue and nt_epilogue_lds on the multi-stage tile kernel implement it:
  // bigdl_conv_addend_stride_applies)
  int add_sh, add_sw, add_H, add_W;
  unsigned add_mow, add_moh, add_msh, add_msw;
};

// int8 convolution epilogue (quant.hip, conv_halo.hip): dequantize with the per-sample input scale and the per-channel
// weight scale, + bias, + an optional int8 residual addend, ReLU, then bf16 / fp32 / requantized int8 stores
struct I8Epi {
  const float* xscale;   // [N] per-sample scale, or nullptr -> xs_const
  float xs_const;
  const float* wscale;   // [Ncol]
  int out_mode;          // 0 bf16, 1 fp32, 2 int8
  float out_inv;         // int8 output: 1 / out_scale
  const int8_t* add8;    // optional int8 residual addend [M][add_ld] (dequantized with add_scale, before the ReLU)
  float add_scale;
  long add_ld;
};

// Which kernel takes a ConvArgs call, and how: the one place this is decided is bigdl_conv_nt_choose. Ids <= 0 launch
// nothing: CONV_NONE (no output rows) succeeds, the negative ones are bigdl_conv_nt's error returns.
enum ConvKernel {
  CONV_ERR_LAUNCH = -8,      // a launcher refused what its own predicate accepted
  CONV_ERR_WORKSPACE = -7,   // ws_floats > 0 and no ConvArgs::ws
  CONV_ERR_ADDEND = -6,      // subsampled addend on a kernel that does not implement it
  CONV_ERR_PRE = -5,         // BN on load on a kernel that does not implement it
  CONV_ERR_WINDOW = -4,      // overlapping-window source the g4 kernel cannot take
  CONV_ERR_OUT32 = -3,
  CONV_ERR_BNRED = -2,
  CONV_ERR_SHAPE = -1,
  CONV_NONE = 0,
  CONV_STEM,                 // 7x7 / stride-2 pair-view stem (stem_fwd.hip)
  CONV_G4,                   // multi-stage LDS-DMA tile: BM x BN, `stages` deep (2 = the short-K form)
  CONV_S1,                   // streaming 1x1
  CONV_HALO,                 // 3x3 from halo tiles (conv_halo.hip)
  CONV_P8_SK,                // 256 x 256 phase-interleaved, stream-K (sk_slots slots per tile)
  CONV_P8_SPLIT,             // ... split over K (ksplit) + split-K epilogue
  CONV_P8,
  CONV_W8_SPLIT,             // 256 x 256 8-wave, split over K + split-K epilogue
  CONV_W8,
  CONV_P3,                   // 256-pixel deep-pipelined 8-wave
  CONV_PERS,                 // persistent LDS-DMA
  CONV_GLDS_ONESTAGE,        // LDS-DMA, Kdim == one K-step
  CONV_GLDS,                 // 2-stage LDS-DMA
  CONV_GLDS_SLOWK,           // ... per-lane taps (Cs % 64 != 0)
  CONV_REG,                  // register-staged
};
struct ConvChoice {
  int kernel;                // ConvKernel
  int BM, BN, stages;        // tile of the kernels that have several launch shapes (0 where there is one)
  int ksplit;                // K split (1 = none)
  int sk_slots;              // stream-K: (tile, segment) slots per tile
  int ktail;                 // P8: one tap with Cs % 64 != 0, granules past Kdim read zeros
  long ws_floats;            // fp32 workspace the caller passes in ConvArgs::ws (0: none)
};

// The same for the int8 convolution (bigdl_conv_i8_choose). Ids <= 0 launch nothing: I8_NONE (no output rows) succeeds,
// the negative ones are bigdl_conv_i8's error returns.
enum I8Kernel {
  I8_ERR_LAUNCH = -2,        // a launcher refused what its own predicate accepted
  I8_ERR_SHAPE = -1,         // Cs % 16 != 0, or Kdim / ntaps out of range
  I8_NONE = 0,
  I8_STEM,                   // 7x7 / stride-2 image stem over its width im2col (conv_halo.hip stem_i8_kernel)
  I8_HALO,                   // 3x3 from halo tiles (conv_halo.hip)
  I8_S1,                     // streaming 1x1: cg 64-channel groups x 4 / cg pixel groups per workgroup
  I8_P8,                     // 256 x 256 phase-interleaved
  I8_G3,                     // multi-stage counted-vmcnt tile: BM x BN, `stages` deep (2 = the short-K form)
  I8_GLDS,                   // 2-stage LDS-DMA tile: BM x BN
};
struct I8Choice {
  int kernel;                // I8Kernel
  int BM, BN;                // tile (0: stem / halo, whose tiles follow the image width)
  int stages, cpl;           // g3: pipeline depth, channels per lane in the epilogue (0 elsewhere)
  int direct;                // g3 / p8: register-direct epilogue
  int fastk;                 // a K-step lies in one tap (g3: Cs % 64 == 0, glds: Cs % 128 == 0)
  int cg;                    // s1: channel groups per workgroup (4, 2 or 1)
};

// The same for the weight gradient (bigdl_conv_wgrad_choose).
enum WgradKernel {
  WGRAD_ERR_LAUNCH = -9,
  WGRAD_ERR_WORKSPACE = -8,
  WGRAD_ERR_PRE_X = -7,      // WgradArgs::pre_x on anything but the pair-view stem kernel
  WGRAD_ERR_PRE = -6,        // WgradArgs::pre on anything but the halo kernel
  WGRAD_ERR_SHAPE = -1,
  WGRAD_STEM = 1,            // pair-view stem (stem_fwd.hip); splits = -1, it splits by workgroup
  WGRAD_HALO,                // 3x3 / stride 1 from halo tiles (wgrad_halo.hip)
  WGRAD_P8_DIRECT,           // 256 x 256 phase-interleaved, 1x1 / stride 1 operands read in place
  WGRAD_P8,
  WGRAD_GLDS_WS,             // 128 x 128 2-stage LDS-DMA, workspace partials + fixed-order reduce
  WGRAD_G3_WS,               // ... 3-stage
  WGRAD_GLDS_ATOMIC,         // the same two adding into dw with fp32 atomics
  WGRAD_G3_ATOMIC,
  WGRAD_REG,                 // register-staged, fp32 atomics
};
struct WgradChoice {
  int kernel;                // WgradKernel
  int splits, m_per_split;   // pixel split (WgradArgs::splits / m_per_split of the launch)
  long ws_floats;            // fp32 workspace the caller passes in WgradArgs::ws (0: none)
};

struct WgradArgs {
  const uint16_t* dy;
  const uint16_t* src;
  float* dw;
  float* dbias;
  int Nb, Hs, Ws, Cs, OH, OW, R, S;
  int sh, sw, ph, pw, dh, dwl;
  int M, Ncol, Kdim, ldy;
  int m_per_split;
  float* ws;       // split-K partials [splits][Ncol][Kdim] (nullptr: fp32 atomics into dw)
  int splits;
  float* det_ws;    // deterministic mode with dbias: BIGDL_DET_SLOTS x Ncol floats for the bias column sum
  // optional [2 Cs] scale | shift: src is the input of a training BN + ReLU, read as relu(src * scale + shift)
  // (ConvArgs::pre semantics; the halo 3x3 weight gradient only: bigdl_wgrad_pre_applies)
  const float* pre;
  // optional, all three or none (the pair-view stem kernel only, bigdl_stem_wgrad): dy is the output gradient dz of
  // the training BN + ReLU that consumes this convolution's output pre_x (bf16, dy's layout), and the convolution's
  // own output gradient A * mask(dz) + B * pre_x + D is formed on load, rounded as bigdl_bn_bwd_apply rounds it.
  // pre_coef: [3 Ncol] A | B | D (bigdl_bn_bwd_apply's coef); pre_aff: [2 Ncol] scale | shift, mask = pre_x * scale + shift > 0
  const uint16_t* pre_x;
  const float* pre_coef;
  const float* pre_aff;
};

extern "C" {
void bigdl_fill_bytes(void* ptr, int value, long bytes, hipStream_t st);
int bigdl_deterministic();
void bigdl_set_deterministic(int v);
// deterministic-mode partial slots (bigdl_colsum_bf16_ld / bigdl_sumsq workspaces: DET_SLOTS x K / DET_SLOTS floats)
#define BIGDL_DET_SLOTS 128
void bigdl_colsum_bf16_ld(const uint16_t* x, float* out, long P, int K, long ld, hipStream_t st,
                          float* det_ws = nullptr);
// Kernel choice for `a`: a pure host function of the args, the BIGDL_CONV_* switches and the device's CU count. It
// launches nothing and tests the pointers of `a` for null / alignment only. A choice with ws_floats > 0 needs that
// many floats in a->ws. CONV_ERR_PRE / CONV_ERR_ADDEND: no kernel that takes the GEMM applies a->pre / the subsampled
// addend (the caller materialises the operand and chooses again).
ConvChoice bigdl_conv_nt_choose(const ConvArgs* a);
// compute units of the current device, read once (conv_igemm.hip)
int conv_cus();
const char* bigdl_conv_kernel_name(int kernel);
// Subsampled addend (ConvArgs::add_sh): bigdl_conv_addend_stride sets the stride, the addend's pixel geometry and the
// reciprocals (sh = sw = 1 switches it off); bigdl_conv_addend_stride_applies is 1 when bigdl_conv_nt_choose accepts
// `a` with it.
void bigdl_conv_addend_stride(ConvArgs* a, int sh, int sw, int add_h, int add_w);
int bigdl_conv_addend_stride_applies(const ConvArgs* a);
// Launches the choice made for `a`; 0 on success, else a negative ConvKernel code.
int bigdl_conv_nt(const ConvArgs* a, const ConvChoice* c, hipStream_t st);
// 3x3 / stride-1 / pad-1 forward or data-gradient GEMM from halo tiles (conv_halo.hip)
int bigdl_conv_halo_applies(const ConvArgs* a);
int bigdl_conv_halo(const ConvArgs* a, hipStream_t st);
void bigdl_set_conv_halo(int v);
// one-pass 3x3 / stride-2 / pad-1 data gradient from halo tiles of dy, all four stride phases in one launch
// (conv_halo.hip; BIGDL_DGRAD_S2, default 1)
int bigdl_dgrad_s2_applies(const ConvArgs* a);
int bigdl_dgrad_s2(const ConvArgs* a, hipStream_t st);
void bigdl_set_dgrad_s2(int v);
// the same on the i8 matrix cores (int8 activations / weights, I8Epi epilogue; no residual addend)
int bigdl_conv_halo_i8_applies(const ConvArgs* a, const I8Epi* ep);
int bigdl_conv_halo_i8(const ConvArgs* a, const I8Epi* ep, hipStream_t st);
// 7x7 / stride-2 pair-view image stem forward (stem_fwd.hip)
int bigdl_stem_fwd_applies(const ConvArgs* a);
int bigdl_stem_fwd(const ConvArgs* a, hipStream_t st);
void bigdl_set_stem_fwd(int v);
long bigdl_stem_wgrad_plan(const WgradArgs* a);
int bigdl_stem_wgrad(const WgradArgs* a, hipStream_t st);
void bigdl_set_stem_wgrad(int v);
// Batched NT GEMM (bmm.hip): C[b][m][n] (=|+=) alpha * sum_k A[b][m][k] B[b][n][k]; A, B bf16 K-contiguous (K % 32
// == 0, row strides % 8 == 0), C fp32. Returns < 0 on unsupported shapes.
int bigdl_bmm_nt(const uint16_t* A, const uint16_t* B, float* C, int batch, int M, int N, int K, long sa, long sb,
                 long sc, int lda, int ldb, int ldc, float alpha, int accum, hipStream_t st);
// Pixel-pair packing for 3/4-channel width-stride-2 stems (stem.hip).
void bigdl_nchw_to_pairs(const float* x, uint16_t* y, int N, int C, int H, int W, int Hp, int Wp, int ph, int pw,
                         hipStream_t st);
void bigdl_pair_weight(const uint16_t* w, uint16_t* wp, int K, int C, int R, int S, const long* strides,
                       hipStream_t st);
void bigdl_pair_wgrad_add(const float* dwp, float* gw, int K, int C, int R, int S, const long* strides, float scale,
                          hipStream_t st);
// Kernel choice and pixel split for the weight gradient (a->splits / m_per_split / ws are not read), and its launch;
// 0 on success, else a negative WgradKernel code.
WgradChoice bigdl_conv_wgrad_choose(const WgradArgs* a);
const char* bigdl_wgrad_kernel_name(int kernel);
// current value of every conv switch that has a setter (tests save and restore them)
int bigdl_get_conv_shortk();
int bigdl_get_conv_p8();
int bigdl_get_conv_w8();
int bigdl_get_conv_sk();
int bigdl_get_conv_s1();
int bigdl_get_wgrad_p8();
int bigdl_get_conv_halo();
int bigdl_get_dgrad_s2();
int bigdl_get_stem_fwd();
int bigdl_get_stem_wgrad();
int bigdl_get_wgrad_halo();
int bigdl_conv_wgrad(const WgradArgs* a, const WgradChoice* c, hipStream_t st);
void bigdl_transpose_krsc(const uint16_t* w, uint16_t* wt, int K, int RS, int C, hipStream_t st);
// batched form: desc = device int64 [n][6] {w ptr, wt ptr, K, RS, C, first tile}, tiles of 32 x 32 per (rs)
void bigdl_transpose_krsc_batched(const long* desc, int n, int total_tiles, hipStream_t st);

// batch norm (NHWC bf16, fp32 statistics). Statistics / backward-reduction buffers are
// [BIGDL_STAT_SLOTS][2][C] fp32, zeroed by the caller; producers add into slot (block id % slots).
#define BIGDL_STAT_SLOTS 128
void bigdl_bn_stats(const uint16_t* x, float* stats, long P, int C, hipStream_t st);
void bigdl_bn_finalize(const float* stats, int nslots, const float* gamma, const float* beta, float* run_mean,
                       float* run_var, float* save_mean, float* save_invstd, float* scale, float* shift,
                       long P, int C, float eps, float momentum, int training, hipStream_t st);
void bigdl_bn_slot_reduce(const float* in, int nslots, int C, float* out, hipStream_t st);
void bigdl_bn_apply(const uint16_t* x, const float* scale, const float* shift, const uint16_t* res,
                    uint16_t* y, long P, int C, int relu, hipStream_t st, uint8_t* zm = nullptr,
                    const float* res_scale = nullptr, const float* res_shift = nullptr);
// res_scale / res_shift (optional, fp32 [C], both or neither): the residual term is bf16(res * res_scale + res_shift),
// i.e. res is the input of a ReLU-less BN whose own apply pass is folded into this one (bit-equal to running it)
// aff (optional, [scale C | shift C] of the forward apply): with z == nullptr the ReLU mask is recomputed from x.
void bigdl_bn_bwd_reduce(const uint16_t* dz, const uint16_t* z, const uint16_t* x, const float* mean,
                         float* red, long P, int C, const float* aff, hipStream_t st, const uint8_t* zm = nullptr);
void bigdl_bn_bwd_apply(const uint16_t* dz, const uint16_t* z, const uint16_t* x, const float* mean,
                        const float* invstd, const float* gamma, const float* red, int nslots, float* coef,
                        uint16_t* dx, uint16_t* dres, float* dgamma, float* dbeta, long P, int C, int training,
                        const float* aff, hipStream_t st, const uint8_t* zm = nullptr,
                        const uint16_t* x2 = nullptr, const float* mean2 = nullptr, float* red2 = nullptr);
// x2 / mean2 / red2: also accumulate the backward reduction of a second (ReLU-less) BN whose output gradient is dres
// (input x2, same layout; mean2) into the slotted red2 (csrc/batchnorm.hip bn_bwd_apply_kernel R2). dres may be null
// there: the sums are taken over the bf16-rounded masked dz whether or not it is stored.
// zm: [P][C / 8] sign bytes of the post-ReLU output (bit e of byte (p, g) = channel 8g + e > 0), written by
// bigdl_bn_apply when non-null and read in place of z by the backward passes (1/16 of z's bytes)

// elementwise
void bigdl_relu_fwd(const uint16_t* x, uint16_t* y, long n, hipStream_t st);
void bigdl_spin_us(double us, int* done, hipStream_t st);
void bigdl_dgrad_fill(uint16_t* out, const uint16_t* add, long npix, int H, int W, int C, int sh, int sw, unsigned mask,
                      hipStream_t st);
void bigdl_relu_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dx, long n, hipStream_t st);
void bigdl_add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* y, long n, hipStream_t st);
void bigdl_nchw_f32_to_nhwc_bf16(const float* x, uint16_t* y, int N, int C, int H, int W, int Cp,
                                 hipStream_t st);
void bigdl_cast_f32_bf16(const float* x, uint16_t* y, long n, hipStream_t st);
void bigdl_colsum_bf16(const uint16_t* x, float* out, long P, int K, hipStream_t st, float* det_ws = nullptr);
// [M][K] bf16 -> [M][K + 8] = [x | 1 | 0...]; gW += sW * gw[:, :K], gB += sB * gw[:, K] (gw [N][K + 8] fp32)
void bigdl_ones_col_pack(const uint16_t* x, uint16_t* xe, long M, int K, hipStream_t st);
void bigdl_ones_col_acc(const float* gw, float* gW, float* gB, long N, int K, float sW, float sB, hipStream_t st);
void bigdl_cast_bf16_f32(const uint16_t* x, float* y, long n, hipStream_t st);

// pooling (NHWC bf16)
void bigdl_maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* idx, int N, int H, int W, int C, int OH,
                       int OW, int kh, int kw, int sh, int sw, int ph, int pw, hipStream_t st, const float* pre = nullptr);
int bigdl_maxpool_pre_applies(int N, int H, int W, int C, int OH, int OW, int kh, int kw, int sh, int sw);
int bigdl_stem_i8_applies(const ConvArgs* a, const I8Epi* ep);
void bigdl_set_stem_i8(int v);
int bigdl_stem_i8_f32(const ConvArgs* a, const I8Epi* ep, const float* img, int C, int W, float inv, hipStream_t st);
int bigdl_stem_i8(const ConvArgs* a, const I8Epi* ep, hipStream_t st);
void bigdl_split_reduce_f32(const float* ws, float* dw, long n, int splits, hipStream_t st);
int bigdl_maxpool_bwd_bnred_applies(int N, int H, int W, int C, int OH, int OW, int kh, int kw, int sh, int sw, int ph,
                                    int pw);
void bigdl_maxpool_bwd_bnred(const uint16_t* dy, const uint8_t* idx, uint16_t* dx, int N, int C, int OH, int OW,
                             const uint16_t* bx, const float* mean, const float* aff, const uint8_t* zm, float* red,
                             hipStream_t st);
void bigdl_maxpool_bwd(const uint16_t* dy, const uint8_t* idx, uint16_t* dx, int N, int H, int W, int C,
                       int OH, int OW, int kh, int kw, int sh, int sw, int ph, int pw, hipStream_t st);
void bigdl_avgpool_fwd(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, int OH, int OW, int kh,
                       int kw, int sh, int sw, int ph, int pw, int count_pad, hipStream_t st);
void bigdl_avgpool_bwd(const uint16_t* dy, uint16_t* dx, int N, int H, int W, int C, int OH, int OW, int kh,
                       int kw, int sh, int sw, int ph, int pw, int count_pad, hipStream_t st);

// fused log-softmax + NLL (cross entropy) over rows of logits
void bigdl_softmax_xent(const uint16_t* logits_bf16, const float* logits_f32, const float* labels,
                        float* loss, uint16_t* dlogits_bf16, float* dlogits_f32, int B, int K,
                        float label_base, float grad_scale, hipStream_t st, float* det_ws = nullptr);
// Deterministic mode with det_ws (BIGDL_XENT_SLOTS floats): the usual grid, every block stores its loss partial to its
// own slot and one wave adds the slots in a fixed order; without det_ws the whole batch runs in one block.
#define BIGDL_XENT_SLOTS 2048

// optimizers over flat fp32 buffers (optional bf16 shadow written in the same pass)
// dampening, beta1, beta2 arrive as doubles: the kernels use 1 - dampening, 1 - beta narrowed once from the double
// difference (1.f - 0.999f is 1.3e-5 off 0.001: 217 fp32 ulps on Adam's second moment)
void bigdl_sgd_step(float* w, const float* g, float* mom, uint16_t* w16, long n, const float* lr_dev, float lr,
                    float wd, float momentum, double dampening, int nesterov, int first, const long* seg_off,
                    const float* seg_wd, int nseg, long base, hipStream_t st);
void bigdl_adam_step(float* w, const float* g, float* m, float* v, uint16_t* w16, long n, float lr,
                     double beta1, double beta2, float eps, float wd, float bc1, float bc2, hipStream_t st);
void bigdl_sumsq(const float* x, float* out, long n, hipStream_t st, float* det_ws = nullptr);
void bigdl_scale_f32(float* x, long n, const float* scale_dev, float scale, hipStream_t st);

// LSTM cell pointwise (gates pre-activations -> c, h), fwd & bwd
void bigdl_lstm_cell_fwd(const float* gates, const float* c_prev, float* c, float* h, float* act, int B,
                         int H, hipStream_t st);
void bigdl_lstm_cell_bwd(const float* act, const float* c_prev, const float* c, const float* dh,
                         const float* dc_next, float* dgates, float* dc_prev, int B, int H, hipStream_t st);

// Int8 inference: per-sample activation quantization (x [N][P][C] bf16 or fp32 -> int8 [N][P][Cp]) and the
// dequantizing implicit-GEMM conv on the i8 MFMA (src/wt are int8 images; out bf16 or fp32).
int bigdl_quantize_act(const void* x, int is_bf16, int8_t* q, float* amax, float* scale, int N, long P, int C,
                       int Cp, int static_amax, hipStream_t st);
// xscale: [N] per-sample activation scales or nullptr (xs_const for the whole tensor); out_mode 0 bf16, 1 fp32,
// 2 int8 requantized with out_inv = 1 / out_scale. Output rows are a->ldo elements apart.
// add8 (optional): int8 residual addend [M][add_ld] with scale add_scale, summed before the ReLU.
// Launches what bigdl_conv_i8_choose chose; 0 on success, else a negative I8Kernel code.
int bigdl_conv_i8(const ConvArgs* a, const float* xscale, float xs_const, const float* wscale, int out_mode,
                  float out_inv, const int8_t* add8, float add_scale, long add_ld, hipStream_t st);
// Kernel choice for an int8 call: a pure host function of the args and the BIGDL_I8_* / BIGDL_STEM_I8 /
// BIGDL_CONV_HALO switches. It launches nothing, queries no device and tests pointers for null / alignment only.
I8Choice bigdl_conv_i8_choose(const ConvArgs* a, const I8Epi* ep);
const char* bigdl_i8_kernel_name(int kernel);
// int8 NHWC pooling (max or average, same scale in and out; output rows ldo apart), graph-input quantizer
// (fp32 NCHW -> int8 NHWC, static scale), bf16 rows -> int8 rows at a channel offset, int8 rows -> bf16.
void bigdl_pool_i8(const int8_t* x, int8_t* y, int N, int H, int W, int Cp, int OH, int OW, int kh, int kw, int sh,
                   int sw, int ph, int pw, int avg, int count_pad, long ldo, hipStream_t st);
void bigdl_quantize_nchw_f32(const float* x, int8_t* q, int N, int C, int HW, int Cp, float inv, hipStream_t st);
void bigdl_quantize_wim2col_f32(const float* x, int8_t* y, int N, int C, int H, int W, int OW, int S, int sw, int pw,
                                float inv, hipStream_t st);
void bigdl_quantize_rows_bf16(const uint16_t* x, int8_t* q, long P, int C, long ldq, float inv, hipStream_t st);
void bigdl_dequantize_rows(const int8_t* q, uint16_t* y, long P, int C, long ld, float scale, hipStream_t st);

// tensor_math.hip: native TensorMath backend (strided apply, reductions, fp32 MFMA GEMM / GEMV)
int bigdl_tensor_apply(float* out, const float* a, const float* b, const float* c, int nd, const long* size,
                       const long* so, const long* sa, const long* sb, const long* sc, int op, float s0, float s1,
                       int contiguous, hipStream_t st);
int bigdl_index_op(int op, float* a, const void* idx, int idx_i64, const float* b, float* out, long outer, long R,
                   long n, long inner, long Rsrc, int* err, hipStream_t st);
void bigdl_masked_fill(float* x, const float* mask, float v, long n, hipStream_t st);
long bigdl_mask_blocks(long n);
void bigdl_mask_scan(const float* mask, long n, int* counts, hipStream_t st);
void bigdl_mask_write(int copy, float* x, const float* mask, const float* src, float* out, long n, const int* counts,
                      long nsrc, hipStream_t st);
int bigdl_topk(const float* x, long outer, long R, long inner, int k, int largest, float* vals, float* inds,
               hipStream_t st);
int bigdl_tensor_reduce(const float* x, long outer, long R, long inner, int op, float p, float* out, float* outi,
                        int mean, float* ws, long chunks, hipStream_t st);
int bigdl_gemm_f32(const float* A, const float* B, const float* Min, float* C, int batch, int M, int N, int K,
                   const long* s, float alpha, float beta, hipStream_t st);
int bigdl_gemv_f32(const float* A, const float* x, const float* Min, float* y, int M, int K, long sam, long sak,
                   long sx, long smi, long sy, float alpha, float beta, hipStream_t st);
void bigdl_copy_rows_i8(const int8_t* src, int8_t* dst, long rows, int C, long lds, long ldd, hipStream_t st);
void bigdl_set_conv_impl(int impl);
void bigdl_set_conv_s1(int v);
void bigdl_set_conv_sk(int v);
// 3x3 / stride 1 / pad 1 weight gradient from halo tiles (wgrad_halo.hip): plan returns its splits (0 = n/a)
void bigdl_set_wgrad_halo(int v);
// LSTM with per-gate dropout masks (lstm_drop.hip)
int bigdl_lstm_drop_rep(const void* x, int x_bf16, long xs_b, long xs_t, uint16_t* y, long ys_g, int B, int T, int K,
                        int Kp, int ones, float p, float mul, unsigned long long seed, long long off, hipStream_t st);
int bigdl_lstm_drop_rep_bwd(const float* dy, long dys_g, int ldy, float* dx, long dxs_b, long dxs_t, const float* add,
                            long as_b, long as_t, int B, int T, int K, float p, float mul, unsigned long long seed,
                            long long off, hipStream_t st);
void bigdl_lstm_pack_gate_w(const float* W, const float* b1, const float* b2, int H, int Kin, int Kp, uint16_t* out,
                            uint16_t* outT, hipStream_t st);
int bigdl_wgrad_halo_plan(WgradArgs* a);
// 1 when bigdl_conv_wgrad applies a->pre on load (the halo kernel takes the GEMM), else the caller materialises src
int bigdl_wgrad_pre_applies(const WgradArgs* a);
int bigdl_wgrad_halo(const WgradArgs* a, hipStream_t st);
int bigdl_get_conv_impl();
void bigdl_set_conv_g4(int v);
void bigdl_set_conv_shortk(int v);
void bigdl_set_conv_p8(int v);
void bigdl_set_conv_w8(int v);
void bigdl_set_wgrad_p8(int v);
int bigdl_get_conv_g4();
void bigdl_set_wgrad_g3(int v);
int bigdl_get_wgrad_g3();
void bigdl_set_wgrad_tr_asm(int v);
int bigdl_get_wgrad_tr_asm();
// the BIGDL_I8_* switches (quant.hip I8Switches)
void bigdl_set_i8_g3(int v);
void bigdl_set_i8_p8(int v);
void bigdl_set_i8_s1(int v);
void bigdl_set_i8_epi(int v);
void bigdl_set_i8_shortk(int v);
void bigdl_set_i8_cpl(int v);
int bigdl_get_i8_g3();
int bigdl_get_i8_p8();
int bigdl_get_i8_s1();
int bigdl_get_i8_epi();
int bigdl_get_i8_shortk();
int bigdl_get_i8_cpl();

// Input pipeline: crop + flip + channel reorder + normalise of a uint8 [N, H, W, 3] BGR batch.
// params: int32 [N][3] = (y0, x0, flip). Output fp32 NCHW [N, 3, OH, OW] or bf16 NHWC [N, OH, OW, 3].
void bigdl_image_augment(const uint8_t* src, const int* params, void* out, int N, int H, int W, int OH, int OW,
                         const float* mean, const float* inv_std, int rgb, int nhwc_bf16, hipStream_t st);
// variable-size batch: resized crop + flip + colour jitter + normalise (csrc/image.hip image_pipeline_kernel);
// offs = int64 byte offset of each image, prm = 16 floats per image (layout in image.hip)
void bigdl_image_pipeline(const uint8_t* src, const long* offs, const float* prm, void* out, int N, int OH, int OW,
                          const float* mean, const float* inv_std, int rgb, int nhwc_bf16, hipStream_t st);

// Detection (csrc/detection.hip): greedy NMS over score-sorted boxes (mask_ws: n * ceil(n/64) uint64),
// RoiAlign forward, RoiPooling forward (argmax) / backward.
int bigdl_nms(const float* boxes_sorted, int n, float thresh, int normalized, int max_keep,
              unsigned long long* mask_ws, int* keep_out, int* count_out, hipStream_t st);
int bigdl_roi_align_fwd(const float* x, const float* rois, float* out, int R, int rcols, int C, int H, int W,
                        int PH, int PW, float scale, int sampling, hipStream_t st);
// Segmented greedy NMS: one workgroup per (image, class) of scores [R][C] / boxes [R][Cb][4] (Cb == C or 1); offsets =
// B + 1 host row offsets. keep [R][C] uint8 is written in full; overflow[0] = 1 when a segment has more candidates
// than the LDS capacity (cap: 0 = chosen from the longest image, else 256, 1024 or 4096). Returns the capacity used,
// or < 0 on a bad argument.
int bigdl_nms_classes(const float* scores, const float* boxes, unsigned char* keep, int* overflow,
                      const int* offsets_host, int B, int C, int Cb, int skip_class, float score_thresh,
                      int inclusive, int pre_topk, float nms_thresh, int normalized, int cap, hipStream_t st);
// RoiAlign over up to 8 pyramid levels in one launch: rois [R][5] (batch index first), levels int32 [R]; both
// indices are clamped to the maps that exist.
#define BIGDL_ROI_MAX_LEVELS 8
struct RoiLevelMaps {
  const float* x[BIGDL_ROI_MAX_LEVELS];
  int H[BIGDL_ROI_MAX_LEVELS], W[BIGDL_ROI_MAX_LEVELS];
  float scale[BIGDL_ROI_MAX_LEVELS];
  int L, N, C;
};
int bigdl_roi_align_levels_fwd(const RoiLevelMaps* maps, const float* rois, const int* levels, float* out, int R,
                               int PH, int PW, int sampling, hipStream_t st);
// Segmented top-k in the order of a stable descending sort (NaN first, -0.0 == +0.0, ties by lower index),
// 1 <= k <= 4096, one workgroup per segment. Flat mode: values [R], mask uint8 [R] or null, S + 1 host offsets into
// values and S + 1 into the outputs (segment s owns min(k, len_s) slots); out_idx is relative to the segment unless
// global_index; counts [S] or null. Slots past a segment's count hold its first index and value 0.
int bigdl_segmented_topk_flat(const float* values, const unsigned char* mask, const int* in_off_host,
                              const int* out_off_host, int S, int k, int global_index, int* out_idx, float* out_val,
                              int* counts, hipStream_t st);
// Level-map mode: segment (n, l) is image n of obj[l] [N][A][H_l][W_l] in (h, w, a) order; besides indices and
// values it gathers the rows of reg[l] [N][4A][H_l][W_l] and anc[l] [H_l W_l A][4] into out_reg / out_anc [slots][4].
struct TopkLevelMaps {
  const float* obj[BIGDL_ROI_MAX_LEVELS];
  const float* reg[BIGDL_ROI_MAX_LEVELS];
  const float* anc[BIGDL_ROI_MAX_LEVELS];
  int HW[BIGDL_ROI_MAX_LEVELS];
  int L, N, A;
};
int bigdl_segmented_topk_maps(const TopkLevelMaps* maps, int k, int* out_idx, float* out_val, float* out_reg,
                              float* out_anc, hipStream_t st);
int bigdl_roi_pool_fwd(const float* x, const float* rois, float* out, int* argmax, int R, int C, int H, int W,
                       int PH, int PW, float scale, hipStream_t st);
int bigdl_roi_pool_bwd(const float* gy, const int* argmax, const float* rois, float* gx, int R, int C, int H, int W,
                       int PH, int PW, hipStream_t st);

// Misc NN kernels (csrc/nn_misc.hip): LRN across channels (NCHW fp32), Philox dropout (mask regenerated in
// backward), embedding gather / atomic scatter-add, TF-style bilinear resize (NCHW fp32), row log-softmax,
// fp32 -> bf16 round-toward-zero (FP16CompressedTensor parity).
void bigdl_lrn_fwd(const float* x, float* y, float* scale, int N, int C, long HW, int size, float alpha, float beta,
                   float k, hipStream_t st);
void bigdl_lrn_bwd(const float* x, const float* y, const float* scale, const float* gy, float* gx, int N, int C, long HW,
                   int size, float alpha, float beta, hipStream_t st);
void bigdl_dropout(const void* x, void* y, int is_bf16, long n, float p, float mul, unsigned long long seed,
                   hipStream_t st);
void bigdl_embedding_fwd(const float* W, const long* idx, float* out, long rows, int D, long nIndex, hipStream_t st);
void bigdl_embedding_fwd_ids(const float* W, const void* ids, int ids_long, float* out, long rows, int D, long nIndex,
                             int mask_zero, hipStream_t st);
void bigdl_embedding_bwd_ids(const void* gout, int gout_bf16, const void* ids, int ids_long, float* gW, long rows, int D,
                             long nIndex, long pad, float scale, hipStream_t st);
void bigdl_embedding_bwd(const float* gout, const long* idx, float* gW, long rows, int D, long nIndex, float scale,
                         hipStream_t st);
// Deterministic-mode embedding gradient: keys = the weight row of every token position, stably sorted (ascending
// position inside a row's run), pos = the matching positions. Every run whose key lies in [0, nIndex) is summed in
// fp32 in that order, one wave per (run, 64-column slice), then gW[key] += scale * sum once. No atomics.
void bigdl_embedding_bwd_sorted(const void* gout, int gout_bf16, const long* keys, const long* pos, float* gW, long rows,
                                int D, long nIndex, float scale, hipStream_t st);
void bigdl_resize_bilinear_fwd(const float* x, float* y, long NC, int H, int W, int OH, int OW, float sh, float sw,
                               hipStream_t st);
void bigdl_resize_bilinear_bwd(const float* gy, float* gx, long NC, int H, int W, int OH, int OW, float sh, float sw,
                               hipStream_t st);
void bigdl_log_softmax_fwd(const float* x, float* y, long rows, int cols, hipStream_t st);
void bigdl_log_softmax_bwd(const float* y, const float* gy, float* gx, long rows, int cols, hipStream_t st);
void bigdl_f32_to_bf16_rtz(const float* x, uint16_t* y, long n, hipStream_t st);

// Sparse COO kernels (csrc/sparse.hip) over a coalesced 2-D tensor [B, D]: rows / cols = the two int64 index rows
// [nnz] in row-major order, vals fp32 [nnz], offs = int32 CSR offsets [B + 1] from bigdl_coo_row_offsets (nnz < 2^31).
// Entries with a row outside [0, B), a column outside [0, D) or an id outside [1, nIndex] contribute nothing.
void bigdl_coo_row_offsets(const long* rows, long nnz, int B, int* offs, hipStream_t st);
// y[b, o] = bias[o] + sum_k val_k W[o, col_k] over row b's entries; W [N, D] as stored, bias [N] or null
void bigdl_spmm_fwd(const long* cols, const float* vals, const int* offs, const float* W, const float* bias, float* y,
                    int B, int N, long D, hipStream_t st);
// gW[o, col_k] += scale val_k gy[row_k, o]: fp32 atomics, or (sorted) keys = the columns stably sorted with -1 for
// entries to skip, pos = the matching entry numbers, one in-order sum and one plain store per (o, column)
void bigdl_spmm_wgrad(const long* rows, const long* cols, const float* vals, const float* gy, float* gW, long nnz,
                      int B, int N, long D, float scale, hipStream_t st);
void bigdl_spmm_wgrad_sorted(const long* keys, const long* pos, const long* rows, const float* vals, const float* gy,
                             float* gW, long nnz, int B, int N, long D, float scale, hipStream_t st);
// g[k] = sum_o gy[row_k, o] W[o, col_k]: the gradient values on the input's own pattern (0 for a skipped entry)
void bigdl_sddmm_rows(const long* rows, const long* cols, const float* gy, const float* W, float* g, long nnz, int B,
                      int N, long D, hipStream_t st);
// out[b, :] = s_b sum_k w_k W[id_k - 1, :]; ids = fp32 1-based ids on the pattern, wts = weights on the same pattern
// or null (w = 1); combiner 0 sum (s = 1), 1 mean (1 / sum w), 2 sqrtn (1 / sqrt(sum w^2)), sums over in-range ids
// only, s = 0 for an empty row; scales [B] receives s_b for the backward.
void bigdl_lookup_sparse_fwd(const int* offs, const float* ids, const float* wts, const float* W, float* out,
                             float* scales, int B, int nOut, long nIndex, int combiner, hipStream_t st);
// gW[id_k - 1, :] += scale s_b w_k gy[b, :]: atomics, or (sorted) keys = id - 1 stably sorted with -1 to skip
void bigdl_lookup_sparse_bwd(const int* offs, const float* ids, const float* wts, const float* scales, const float* gy,
                             float* gW, int B, int nOut, long nIndex, float scale, hipStream_t st);
void bigdl_lookup_sparse_bwd_sorted(const long* keys, const long* pos, const long* rows, const float* wts,
                                    const float* scales, const float* gy, float* gW, long nnz, int B, int nOut,
                                    long nIndex, float scale, hipStream_t st);
// Join of up to 8 coalesced inputs [B, D_i] along the columns: output row b = the inputs' row-b segments in input
// order with columns shifted by shift[i] = sum_{j<i} D_j. total = sum of the inputs' nnz = the output's capacity.
#define BIGDL_SPARSE_MAX_JOIN 8
struct SparseJoinInputs {
  const long* cols[BIGDL_SPARSE_MAX_JOIN];
  const float* vals[BIGDL_SPARSE_MAX_JOIN];
  const int* offs[BIGDL_SPARSE_MAX_JOIN];
  long shift[BIGDL_SPARSE_MAX_JOIN];
  int n;
};
int bigdl_sparse_concat_cols(const SparseJoinInputs* in, int B, long* out_rows, long* out_cols, float* out_vals,
                             long total, hipStream_t st);

// Fused LSTM steps (csrc/lstm.hip) with optional peepholes, optional row mask and a caller-given gate layout. W16
// [4H][H] bf16, WT16 = W^T [H][4H] bf16. Row strides: xg/h_out/acts/dout/dg_out rows are batch rows (ldx, ldh, lda,
// ldd, ldg elements apart). gi, gf, gg, go: positions (a permutation of 0..3) of the i, f, g, o blocks in the [4H]
// gate axis of xg / W16 / acts / dg; nn.LSTM's blocks i, g, f, o are (0, 2, 1, 3). pI, pF, pO fp32 [H], all three or
// none. mask: this step's [B] bytes, 1 = valid row, or null. h_state (fp32 [B, H], in place, may be null) and carry
// (fp32 [B, H], in place, required with a mask) hold what a masked row passes on. With nn.LSTM's layout and every
// optional pointer null the specialised instantiation runs. Return -1 on an unsupported argument.
int bigdl_lstm_fwd_step(const uint16_t* W16, const uint16_t* h16_prev, const float* xg, long ldx, const float* c_prev,
                        float* c_out, float* h_state, float* h_out, long ldh, uint16_t* h16_out, float* acts, long lda,
                        const float* pI, const float* pF, const float* pO, const unsigned char* mask, int gi, int gf,
                        int gg, int go, int B, int H, hipStream_t st);
int bigdl_lstm_bwd_step(const uint16_t* WT16, const uint16_t* dg16_next, const float* dout, long ldd,
                        const float* dh_ext, const float* acts, long lda, const float* c_prev, const float* c_t,
                        float* dc, float* carry, float* dg_out, long ldg, uint16_t* dg16_out, const float* pI,
                        const float* pF, const float* pO, const unsigned char* mask, int gi, int gf, int gg, int go,
                        int B, int H, hipStream_t st);
// Peephole weight gradients out[3][H] = (dp_i, dp_f, dp_o) from the saved fp32 gate gradients dg (element (b, t, k) at
// b * dg_sb + t * dg_st + k) and cell states cs [T, B, H] / c0 [B, H]; part is a [slices(T * B)][3][H] workspace.
// Fixed summation order, no atomics.
int bigdl_lstm_peep_wgrad_slices(long rows);
int bigdl_lstm_peep_wgrad(const float* dg, long dg_sb, long dg_st, const float* cs, const float* c0, float* part,
                          float* out, int gi, int gf, int gg, int go, int T, int B, int H, hipStream_t st);
// Whole-sequence persistent LSTM (csrc/lstm_seq.hip): one launch per direction, W resident in VGPRs.
int bigdl_lstm_seq_supported(int B, int H);
void bigdl_set_lstm_seq(int v);
int bigdl_lstm_seq_sync_words();
int bigdl_gru_seq_supported(int B, int H);
int bigdl_gru_seq(int bwd, const uint16_t* Wrz16, const uint16_t* Wn16, const float* xg, const float* h0,
                  uint16_t* h16, uint16_t* rh16, float* gates, float* out, const float* dout, const float* dhT,
                  float* dx, uint16_t* dn16, uint16_t* drz16, float* dh0, unsigned* sync, int B, int H, int T,
                  hipStream_t st);
int bigdl_persistent_error(int clear);
unsigned* bigdl_host_word_dev(int slot);
int bigdl_host_word(int slot, int clear);
void bigdl_set_seq_timeout_us(double us);
void bigdl_hog_cus(int n, double us, int* done, hipStream_t st);
unsigned* bigdl_persistent_err_dev();
unsigned long long bigdl_seq_spin_ticks();
int bigdl_lstm_seq_fwd(const uint16_t* W16, const void* xg, const float* c0, uint16_t* h16, void* out, float* hT,
                       float* cs, float* acts, unsigned* sync, int B, int H, int T, int bf16io, hipStream_t st);
int bigdl_lstm_seq_bwd(const uint16_t* W16, const void* dout, const float* dhT, const float* dcT, const float* acts,
                       const float* cs, const float* c0, uint16_t* dg16, void* dxg, float* dc0, float* dh0,
                       unsigned* sync, int B, int H, int T, int bf16io, hipStream_t st);

// Fused GRU steps (csrc/gru.hip). mode: 0 fwd r/z, 1 fwd n + h, 2 bwd dh_t + dn/dz, 3 bwd dr + r-path, 4 bwd dh_0.
// GEMM D[b][n] = sum_k A[b][k] W[n][k] (A rows lda apart; W [N][K] contiguous); row strides of the fp32 per-step
// views (xg, hprev, hout, dout, dx) are in elements; every other buffer is a contiguous [B][H] ([B][2H] drz16).
typedef struct {
  const uint16_t* A; long lda; const uint16_t* W; int B, H, K, N, mode;
  const float* xg; long ldx; const float* hprev; long ldhp; float* r; float* z; float* n; uint16_t* rh16;
  float* hout; long ldho; uint16_t* h16out; const float* dout; long ldd; float* dhp; float* dx; long lddx;
  uint16_t* dn16; uint16_t* drz16; float* dh0;
} GruStepArgs;
int bigdl_gru_step(const GruStepArgs* a, hipStream_t st);

// Layer normalisation over the last dimension (csrc/layernorm.hip), D <= 4096, fp32 rows.
int bigdl_layernorm_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, long rows,
                        int D, float eps, hipStream_t st);
int bigdl_layernorm_bwd(const float* dy, const float* x, const float* g, const float* mean, const float* rstd,
                        float* dx, float* dg, float* db, long rows, int D, float* det_ws, hipStream_t st);
// Row chunks of the parameter-gradient pass, a function of (rows, D) only. In deterministic mode the caller passes
// det_ws, chunks x 2 x D floats: every chunk stores its partial sums there and one pass adds them up in chunk order.
long bigdl_layernorm_param_chunks(long rows, int D);

// Fused attention (csrc/attention.hip). q/k/v bf16 [BH][L][D] (D = 32, 64, 96 or 128), bias fp32 through element
// strides (sb, sh, sq, sk) or nullptr, o / dq / dk / dv / dout fp32, lse / delta fp32 [BH][Lq] (lse is an output only); attention dropout
// with probability drop_p (0: none) from a counter-based hash of (seed, row, key), regenerated by the backward.
typedef struct {
  const uint16_t* q; const uint16_t* k; const uint16_t* v; const float* bias; long sb, sh, sq, sk;
  float* o; float* lse; const float* dout; const float* delta; float* dq; float* dk; float* dv;
  float* mlog;   // fp32 [2][BH][Lq]: row max and log row sum (lse's two terms), written by fwd, read by bwd
  int BH, H, Lq, Lk, D, causal;
  float drop_p; unsigned long long seed;
} AttnCall;
int bigdl_attn_fwd(const AttnCall* c, hipStream_t st);
int bigdl_attn_bwd(const AttnCall* c, float* delta_ws, hipStream_t st);
// dQ route of bigdl_attn_bwd (BIGDL_ATTN_DQ=atomic|ordered): -1 unset, 0 atomic, 1 ordered. Unset and atomic mean the
// fp32-atomic sum over key blocks, except in deterministic mode, which always takes the ordered kernel. The ordered
// kernel overwrites dq (no zero fill needed). bigdl_attn_dq_ordered(): 1 if the next call takes the ordered kernel.
void bigdl_set_attn_dq(int v);
int bigdl_attn_dq_ordered();

// Single-token attention decode and KV-cache maintenance (csrc/attn_decode.hip). q / o fp32 [N][heads * D] (q already
// scaled; rounded to bf16 on load), kcache / vcache bf16 [R][Lmax][heads * D], keys 0..len-1 valid, rows (optional,
// int32 [N]) the cache row of sequence n (clamped to [0, R)), bias (optional) fp32 [R][Lmax] read through the same
// rows. D = 32, 64, 96 or 128. kv_append writes the fp32 rows k, v [N][hidden] to position pos of both caches
// ([N][Lmax][hidden]) as bf16. kv_reorder: dst[x][n][0..len) = src[x][parent[n]][0..len) over planes x of
// [N][Lmax][hidden] (src != dst). Return -1 on an unsupported argument.
int bigdl_attn_decode(const float* q, const uint16_t* kcache, const uint16_t* vcache, const int* rows,
                      const float* bias, float* o, int N, int R, int Lmax, int heads, int D, int len, hipStream_t st);
int bigdl_kv_append(const float* k, const float* v, uint16_t* kcache, uint16_t* vcache, int N, int Lmax, int hidden,
                    int pos, hipStream_t st);
int bigdl_kv_reorder(const uint16_t* src, uint16_t* dst, const int* parent, int planes, int N, int Lmax, int hidden,
                     int len, hipStream_t st);

// Adaptive OptimMethod updates on flat fp32 buffers (csrc/optim.hip): method 0 Adagrad (a = lr, b = weight decay),
// 1 RMSprop (a = lr, b = decay rate, c = eps), 2 Adadelta (a = decay rate, b = eps), 3 Adamax (a = lr / (1 - b1^t),
// b = b1, c = b2, d = eps), 4 Ftrl (a = lr, b = lr power, c = l1, d = l2, e = l2 shrinkage); s1 / s2 are the state
// buffers (s2 may be null for Adagrad / RMSprop); w16 (optional) receives the bf16 copy of the updated weights.
// om = 1 - decay rate of the moving average (RMSprop 1 - b, Adadelta 1 - a, Adamax 1 - b), narrowed from the double
// difference by the caller.
typedef struct { float a, b, c, d, e, om; } OptimHP;
int bigdl_optim_step(int method, const OptimHP* hp, float* x, const float* g, float* s1, float* s2, uint16_t* w16,
                     long n, hipStream_t st);

// Fused LARS over every layer at once (csrc/lars.hip). A *piece* is [lo, hi) of the flat fp32 buffers and belongs to
// one layer; a *chunk* is up to BIGDL_LARS_CHUNK consecutive elements of one piece. Tables (device memory):
// chunk_piece int32 [nchunks], chunk_start int64 [nchunks] (absolute element index), piece_tab int64 [npieces][4] =
// (lo, hi, momentum offset - lo, layer), piece_hp fp32 [npieces][2] = (weight decay, momentum), layer_chunks int32
// [nlayers][2] = [first chunk, end chunk). w, g, v (and w16) must share one 16-byte phase: (address / element size)
// mod 4 is the same for all of them (-1 otherwise), so that one head / 16-byte body / tail split serves them all.
// bigdl_lars_norms: ws[2 c], ws[2 c + 1] = sum w^2, sum g^2 of chunk c (plain stores), then acc[2 l], acc[2 l + 1] =
// the sums of layer l's chunks in a fixed order (0 for a layer without a chunk): two launches, no atomics.
// bigdl_lars_update: scale = guard((sqrt(acc g) + WD sqrt(acc w)) / sqrt(acc w)), rate = rates[piece] / scale,
// v = momentum v + (g + wd w) rate, w -= v, w16 = bf16(w) (w16 optional): one launch.
#define BIGDL_LARS_CHUNK 4096
#define BIGDL_LARS_BLOCK_CAP 2048
int bigdl_lars_norms(const float* w, const float* g, const int* chunk_piece, const long* chunk_start,
                     const long* piece_tab, const int* layer_chunks, float* ws, float* acc, int nchunks, int nlayers,
                     hipStream_t st);
int bigdl_lars_update(float* w, const float* g, float* v, uint16_t* w16, const int* chunk_piece,
                      const long* chunk_start, const long* piece_tab, const float* piece_hp, const float* rates,
                      const float* acc, double WD, int nchunks, hipStream_t st);

// Point-wise activations (csrc/activation.hip): kind codes in bigdl_amd/nn/activation.py _NATIVE_KIND; x, y, dy, dx
// are contiguous bf16 (bf16 = 1) or fp32 buffers of n elements; returns -1 for an unknown kind.
int bigdl_act_fwd(const void* x, void* y, long n, int bf16, int kind, float a, float b, hipStream_t st);
int bigdl_act_bwd(const void* x, const void* y, const void* dy, void* dx, long n, int bf16, int kind, float a,
                  float b, hipStream_t st);

// N-d window pooling / nearest up-sampling (csrc/pool_nd.hip) over a dense [B][D][H][W][C] view (C innermost):
// input D x H x W, output OD x OH x OW, window (kd, kh, kw), stride, padding (for up-sampling kd / kh / kw are the
// integer scale factors and stride / padding are unused). idx (max pooling) holds the input position (d*H+h)*W+w.
typedef struct { int B, D, H, W, C, OD, OH, OW, kd, kh, kw, sd, sh, sw, pd, ph, pw; } PoolNdGeo;
int bigdl_poolnd_fwd(const void* x, void* y, int* idx, const PoolNdGeo* g, int max_mode, int count_pad, int bf16,
                     hipStream_t st);
int bigdl_poolnd_bwd(const void* dy, const int* idx, void* dx, const PoolNdGeo* g, int max_mode, int count_pad,
                     int bf16, hipStream_t st);
int bigdl_upsample_nearest(const void* src, void* dst, const PoolNdGeo* g, int backward, int bf16, hipStream_t st);

// Direct grouped / depthwise convolution, fp32 NCHW (csrc/grouped_conv.hip). pass 0 forward (x, w, b -> y),
// 1 data gradient (dy, w -> dx), 2 weight / bias gradient (dy, x -> dwt, db accumulated).
typedef struct {
  const float* x; const float* w; const float* b; float* y; const float* dy; float* dx; float* dwt; float* db;
  int N, C, H, W, K, OH, OW, R, S, sh, sw, ph, pw, dh, dw, G;
} GConvCall;
int bigdl_gconv(const GConvCall* c, int pass, hipStream_t st);

// Dense bf16 GEMM (gemm_bf16.hip): C = alpha * op(A) * op(B) + bias[n] + beta * C over row-major bf16 operands.
// form 0 NT: A[M,K], B[N,K]; 1 NN: A[M,K], B[K,N]; 2 TN: A[K,M], B[K,N] (K = the reduction length in every form).
// Inner extents and leading dimensions (elements) are multiples of 8, bases 16-byte aligned. c is fp32 (beta
// allowed) or bf16; bias (NT / NN) fp32 or bf16 of N; colsum (TN) fp32 of M: colsum[m] += colscale * sum_k A[k][m].
// ws: bigdl_gemm_bf16_ws_bytes(form, M, N, K) bytes (0 when the reduction is not split). The *_bytes / kt_per
// fields are filled by the host entry.
typedef struct {
  const uint16_t* a;
  const uint16_t* b;
  void* c;
  const void* bias;
  float* colsum;
  float* ws;
  int form, M, N, K;
  int lda, ldb, ldc;
  int out_bf16, bias_bf16;
  float alpha, beta, colscale;
  unsigned a_bytes, b_bytes, c_bytes;
  int kt_per;
} GemmBf16Args;
size_t bigdl_gemm_bf16_ws_bytes(int form, int M, int N, int K);
int bigdl_gemm_bf16(const GemmBf16Args* a, size_t ws_bytes, hipStream_t st);
}
