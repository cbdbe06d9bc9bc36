/*
 * matrix_eyes_hip_ops.h — kernel-level entry points of libmatrixeyes_hip.so.
 *
 * Not part of the drop-in boundary (matrix_eyes_hip.h is): these expose the individual HIP
 * kernels so that parity tests can check each one against the CPU oracle and bench.py can time
 * the dominant kernel against its roofline.  All pointers are DEVICE pointers; 16-bit operands
 * are in the context's dtype (ME_DTYPE_F16 / ME_DTYPE_BF16); work is enqueued on the context's
 * stream and not synchronised.
 *
 * The extents contract (tests/test_gpu_redzone.py holds every entry below to it, each pointer between guard regions of
 * NaN and of zero): no entry's result depends on bytes outside the extents its comment gives for an operand -- a kernel
 * may clamp, mask or over-read inside its tile, but what it reads out there must not reach an output; no entry writes
 * outside the extents of its outputs; and the elements an output's comment documents as not written (the border of a
 * zero-bordered map, the cls rows of me_op_patch_embed, rows of no window in the _segments entries, the foreign
 * channels of a pixel_stride slice, the first header_bytes of me_op_ply_pack, the scale bytes of the rows behind the
 * last one in an activation-layout scale tile) are not touched.
 */
#ifndef MATRIX_EYES_HIP_OPS_H
#define MATRIX_EYES_HIP_OPS_H

#include "matrix_eyes_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ME_ACT_NONE = 0, ME_ACT_GELU = 1, ME_ACT_RELU = 2 };

/* Linear (vit.rs:60-62,74,120,122): out = act(A[M][K] . W[N][K]^T + bias); out16 and/or out32
   [M][N].  tile_cfg -1 = automatic. */
int32_t me_op_linear(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, const void* W16,
                     const float* bias, void* out16, float* out32, int32_t act, int32_t tile_cfg);
/* Block residual update (vit.rs:165-169): x[M][N] += gamma[n] * (A . W^T + bias)  in place. */
int32_t me_op_linear_residual(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16,
                              const void* W16, const float* bias, const float* gamma, float* x32,
                              int32_t tile_cfg);
/* Attention (vit.rs:58-75): qkv16 [windows*tokens][3*heads*64] -> out16 [windows*tokens][heads*64] */
int32_t me_op_attention(me_ctx* ctx, const void* qkv16, void* out16, int32_t windows, int32_t tokens,
                        int32_t heads);
/* The form the forward pass runs (pipeline.hip): the qkv linear writes its first `qcols` output columns (Q) multiplied
   by `qscale` = 1/sqrt(64) * log2(e) -- out16 = round16((A . W^T + bias) * qscale) there, one rounding -- and the
   attention kernel takes that Q as it is (its softmax runs on exp2 with the reference point inside the MFMA
   accumulator).  me_op_attention scales a plain Q itself, with a second rounding. */
int32_t me_op_linear_scaled_cols(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, const void* W16,
                                 const float* bias, void* out16, int32_t qcols, float qscale, int32_t tile_cfg);
int32_t me_op_attention_prescaled(me_ctx* ctx, const void* qkv16, void* out16, int32_t windows, int32_t tokens,
                                  int32_t heads);
/* LayerNorm (vit.rs:165,168,343): x32 [rows][dim] -> y16 and/or y32 */
int32_t me_op_layernorm(me_ctx* ctx, const float* x32, const float* weight, const float* bias,
                        void* y16, float* y32, int64_t rows, int32_t dim, float eps);
/* Conv2d k x k (k in {1,3}, padding (k-1)/2, stride in {1,2}) as implicit GEMM.
   in16b: zero-bordered NHWC [B][H+2][W+2][Cin]; w16: packed [Cout][k*k][Cin];
   out32 [B*Ho*Wo][Cout] and/or out16 (zero-bordered [B][Ho+2][Wo+2][Cout] when border16);
   res32/res32b optional f32 residuals [B*Ho*Wo][Cout]; act applies to out16 (and to out32 when
   act_both). */
int32_t me_op_conv2d(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin,
                     const void* w16, int32_t Cout, int32_t k, int32_t stride, const float* bias,
                     const float* res32, const float* res32b, float* out32, void* out16,
                     int32_t border16, int32_t act, int32_t act_both, int32_t tile_cfg);
/* The depth head's last layers (mod.rs:83-94,329-362): relu(conv3x3(in, w16 [Cmid][9][Cin]) + bias) . w2 + b2, ReLU,
   / f_norm[b] (null: not divided), clamp -> out32 [B][H][W].  in16b: zero-bordered NHWC.  tile_cfg -1: the halo kernel
   (csrc/head_conv.hip) where the shape is the model's (Cin 128, Cmid 32, H % 12 == 0, W % 16 == 0), the implicit-GEMM
   tile elsewhere; >= 0: the implicit-GEMM tile. */
int32_t me_op_head_final(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* w16,
                         int32_t Cmid, const float* bias, const float* w2, const float* b2, const float* f_norm,
                         float clamp_lo, float clamp_hi, float* out32, int32_t tile_cfg);
/* ConvTranspose2d(2,2,stride 2): in16 NHWC [B*H*W][Cin]; w16 packed [(dy*2+dx)*Cout + co][Cin];
   out32 [B][2H][2W][Cout] and/or out16 (zero-bordered when border16).  Cout: any multiple of 4 (every store is four
   channels of one sub-pixel; ME_ERR_BAD_SHAPE otherwise). */
int32_t me_op_conv_transpose2x2(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                int32_t Cin, const void* w16, int32_t Cout, const float* bias,
                                float* out32, void* out16, int32_t border16, int32_t tile_cfg);
/* The 16-bit output forms of the split-operand stages (model.h SplitStage; pipeline.hip conv / linear / convt), which
   me_op_conv2d, me_op_linear and me_op_conv_transpose2x2 cannot ask for.  A split value is the pair hi = T(v),
   lo = T(v - hi) (0 where hi overflowed).  The INPUT side of a split stage needs no entry point: the kernel only sees K
   (or Cin) doubled or tripled against weights stored with every run of K (or Cin) values followed by a copy of itself
   (weights.hip), and the caller builds those operands.
   me_op_conv2d_forms: me_op_conv2d with out16_parts = 1: out16 pixels of Cout (plain), 2: [hi | lo] of 2 Cout,
   3: [hi | lo | hi] of 3 Cout; each zero-bordered when border16.  Cin is the operand's channel count as stored.
   me_op_linear_split: me_op_linear with out16 rows of [hi | lo], 2 N wide.
   me_op_conv_transpose2x2_forms: me_op_conv_transpose2x2 with act16 on the 16-bit copy, out16 pixels pixel_stride
   channels apart (0: Cout, or 2 Cout when out_split: a channel slice of a wider map otherwise) and, when out_split,
   the lo part lo_off channels behind the hi part (0: Cout).  Cin is the operand row's length as stored. */
int32_t me_op_conv2d_forms(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin,
                           const void* w16, int32_t Cout, int32_t k, int32_t stride, const float* bias,
                           const float* res32, const float* res32b, float* out32, void* out16,
                           int32_t border16, int32_t out16_parts, int32_t act, int32_t act_both, int32_t tile_cfg);
int32_t me_op_linear_split(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, const void* W16,
                           const float* bias, void* out16, float* out32, int32_t act, int32_t tile_cfg);
int32_t me_op_conv_transpose2x2_forms(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                      int32_t Cin, const void* w16, int32_t Cout, const float* bias,
                                      float* out32, void* out16, int32_t border16, int32_t act16,
                                      int32_t out_split, int32_t pixel_stride, int32_t lo_off, int32_t tile_cfg);
/* me_op_conv_transpose2x2_forms on operand rows whose last part repeats their first ([hi | lo | hi] against weights stored
   [W_hi | W_hi | W_lo]): the rows are stored a_wrap channels wide (a multiple of 64, at least Cin / 2) and channels
   a_wrap .. Cin - 1 are read from the row's start -- the same K order, the repeated part neither stored nor read.
   a_wrap 0: me_op_conv_transpose2x2_forms itself. */
int32_t me_op_conv_transpose2x2_forms_wrap(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                           int32_t Cin, int32_t a_wrap, const void* w16, int32_t Cout, const float* bias,
                                           float* out32, void* out16, int32_t border16, int32_t act16,
                                           int32_t out_split, int32_t pixel_stride, int32_t lo_off, int32_t tile_cfg);
/* Two ConvTranspose2d(2,2,stride 2) over the same [B][H][W] grid onto the same [B][2H][2W][Cout] map, summed in ONE accumulator
   by one launch (csrc/gemm_core.h gemm_pp_kernel<..., CHAIN>): the K loop of (in16_a [B*H*W][Cin_a], w16_a) from zero, then
   out16 = act16(acc) (zero-bordered when border16) from the accumulators -- the 16-bit output of
   me_op_conv_transpose2x2_forms on set a alone, bit for bit --, then the K loop of (in16_b, w16_b) on top and
   out32 = acc + bias_b.  Cin_b is the K set b walks, a_wrap_b as in me_op_conv_transpose2x2_forms_wrap.  Cin_a, Cin_b:
   multiples of 64, at least 128.  grid_cap: at most that many workgroups (a multiple of 8; 0: no cap).  tile_cfg: only
   configuration 0 (256x256x64/8w-pp) has the chained form; any other answers ME_ERR_BAD_ARG. */
int32_t me_op_conv_transpose2x2_pair(me_ctx* ctx, int32_t B, int32_t H, int32_t W, int32_t Cout, const void* in16_a, int32_t Cin_a,
                                     const void* w16_a, const void* in16_b, int32_t Cin_b, int32_t a_wrap_b, const void* w16_b,
                                     const float* bias_b, float* out32, void* out16, int32_t border16, int32_t act16, int32_t grid_cap,
                                     int32_t tile_cfg);
/* Patch embed + pos (vit.rs:287-295; gemm_core.h EPI_PATCH_EMBED): patches16 [windows * P][768] . W16 [C][768]^T + bias
   + pos[1 + p] -> rows 1 .. P of each window of tokens32 [windows][P + 1][C]; the cls rows are not written
   (me_op_cls_rows writes them). */
int32_t me_op_patch_embed(me_ctx* ctx, const void* patches16, int32_t windows, int32_t P, int32_t C, const void* W16,
                          const float* bias, const float* pos, float* tokens32, int32_t tile_cfg);
/* The layout and element-wise kernels between the GEMMs (csrc/elementwise.hip), one entry point each; arguments as the
   forward pass gives them (pipeline.hip).  grid: a multiple of 8 up to 64 (what me_ctx_create admits).
   me_op_bilinear: src32 [planes][in][in] -> dst16 [planes][out][out] (encoder.rs:125-140).
   me_op_patchify: the 25 + 9 + 1 windows of x0 [B][3][64 g]^2, x1 [B][3][32 g]^2, x2 [B][3][16 g]^2 (16-bit) as im2col
   rows patches [(b * 35 + win) * g * g + py * g + px][c * 256 + iy * 16 + ix]; me_op_patchify_windows: the same for a
   stack of whole windows xs16 [windows][3][16 g]^2.
   me_op_cls_rows: tokens [windows][tpw][dim] row 0 = cls + pos[0 .. dim).
   me_op_merge: reshape_feature + merge (encoder.rs:158-208) as one row gather from tokens [batch * wpi][g * g + 1][dim]
   (ONE of src32 / src16) of windows win0 .. win0 + steps^2 - 1 of each image -> dst16 NHWC [batch][side][side][dim],
   side = g (steps 1) or 2 (g - padding) + (steps - 2)(g - 2 padding); split (src32 only): pixels of [hi | lo], 2 dim.
   me_op_nchw32_to_nhwc: src [B][C][H][W] f32 -> dst32 [B][H][W][C] and/or dst16 (zero-bordered [B][H+2][W+2] when
   border; ReLU when relu16; pixels of [hi | lo] when split).  me_op_nhwc16_to_nchw32 / me_op_nhwc32_to_nchw32: back
   (split: value = hi + lo).  me_op_nhwc32_to_16b: f32 NHWC -> the interior of a bordered 16-bit map, C % 4 == 0.
   me_op_concat_channels: a [pixels][Ca] and b [pixels][Cb] (16-bit, multiples of 8) -> dst [pixels][Ca + Cb].
   me_op_fov_add: dst16b [B][g+2][g+2][C] interior = T(lin[b][1 + p][c] + low[b][p][c]) (fov.rs:66-74), lin [B][tpw][C].
   me_op_fov_final: fov_deg[b] (may be NULL) = x16[b][0 .. k*k*C) . w + bias[0], f_norm[b] = tan(fov_deg/2 in rad)/0.5. */
int32_t me_op_bilinear(me_ctx* ctx, const float* src32, void* dst16, int32_t planes, int32_t in_size, int32_t out_size,
                       int32_t align_corners);
int32_t me_op_patchify(me_ctx* ctx, const void* x0, const void* x1, const void* x2, void* patches, int32_t batch,
                       int32_t grid);
int32_t me_op_patchify_windows(me_ctx* ctx, const void* xs16, void* patches, int32_t windows, int32_t grid);
int32_t me_op_cls_rows(me_ctx* ctx, float* tokens, const float* cls, const float* pos, int32_t windows, int32_t tpw,
                       int32_t dim);
int32_t me_op_merge(me_ctx* ctx, const float* src32, const void* src16, void* dst16, int32_t batch, int32_t wpi,
                    int32_t win0, int32_t steps, int32_t padding, int32_t grid, int32_t dim, int32_t split);
int32_t me_op_nchw32_to_nhwc(me_ctx* ctx, const float* src, float* dst32, void* dst16, int32_t batch, int32_t H,
                             int32_t W, int32_t C, int32_t border, int32_t relu16, int32_t split);
int32_t me_op_nhwc16_to_nchw32(me_ctx* ctx, const void* src16, float* dst, int32_t batch, int32_t H, int32_t W,
                               int32_t C, int32_t border, int32_t split);
int32_t me_op_nhwc32_to_nchw32(me_ctx* ctx, const float* src, float* dst, int32_t batch, int32_t H, int32_t W,
                               int32_t C);
int32_t me_op_nhwc32_to_16b(me_ctx* ctx, const float* src, void* dst16b, int32_t batch, int32_t H, int32_t W,
                            int32_t C, int32_t relu);
int32_t me_op_concat_channels(me_ctx* ctx, const void* a16, const void* b16, void* dst16, int64_t pixels, int32_t Ca,
                              int32_t Cb);
int32_t me_op_fov_add(me_ctx* ctx, const float* lin, const float* low, void* dst16b, int32_t batch, int32_t grid,
                      int32_t C, int32_t tpw);
int32_t me_op_fov_final(me_ctx* ctx, const void* x16, const float* w, const float* bias, float* fov_deg, float* f_norm,
                        int32_t batch, int32_t k, int32_t C);
/* MX block-scaled fp8 (ME_DTYPE_FP8, BASELINE configs[3]; csrc/gemm_fp8.hip, mx_fp8.h).
   me_op_quantize_fp8: f16 [rows][K] -> e4m3 bytes dst8 [rows][K] + one e8m0 scale per 32 K elements into
   `scales`, in the weight operand's layout (weight_layout = 1: rows a multiple of 64, rows*K/32 bytes) or the
   activation operand's (0: ceil(rows/128)*128*K/32 bytes).  me_op_scale_index gives the byte position of
   (row, K block) in either layout, so that a test can read the scales back.
   me_op_layernorm_fp8: LayerNorm with the result quantised as an activation operand.
   me_op_linear_fp8: out = act(A8 . W8^T + bias) with M, N multiples of 256 and K a multiple of 128 (>= 256), as
   ONE of: out16 (f16 [M][N]); out8 + out8_scale (GELU'd, quantised as the next GEMM's activation operand);
   x32 (+ gamma): the residual update x += gamma * (A . W^T + bias). */
int32_t me_op_quantize_fp8(me_ctx* ctx, const void* src16, int64_t rows, int32_t K, int32_t weight_layout,
                           uint8_t* dst8, uint8_t* scales);
int64_t me_op_scale_index(int64_t row, int32_t kblock, int64_t rows, int32_t weight_layout);
int32_t me_op_layernorm_fp8(me_ctx* ctx, const float* x32, const float* weight, const float* bias, uint8_t* y8,
                            uint8_t* yscale, int64_t rows, int32_t dim, float eps);
int32_t me_op_linear_fp8(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale,
                         const uint8_t* W8, const uint8_t* w_scale, const float* bias, void* out16, uint8_t* out8,
                         uint8_t* out8_scale, const float* gamma, float* x32);
/* me_op_linear / me_op_linear_residual over up to three row segments with their own weights, as the encoder's merged
   ViT launches run them (pipeline.hip MergedVit): rows [0, seg1) use W16[0] / bias[0] (/ gamma[0]), [seg1, seg2) the [1]
   set, [seg2, M) the [2] set; seg2 == 0: two segments, seg1 == 0: one.  x32 given: the residual form (gamma taken);
   otherwise out16 = act(A . W^T + bias).  Segment boundaries must be multiples of the tile height of tile_cfg, except
   for the 352-row tile (tile_cfg 10), which lays its row tiles out per segment. */
int32_t me_op_linear_segments(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1, int32_t seg2,
                              const void* const W16[3], const float* const bias[3], const float* const gamma[3],
                              void* out16, float* x32, int32_t act, int32_t tile_cfg);
/* The residual update of me_op_linear_segments with the LayerNorm of the next sublayer in the same launch (the form
   the forward pass runs, vit.rs:165-169; csrc/gemm_core.h resid_ln_epilogue): x32[M][N] += gamma * (A W^T + bias) in
   place and xn16[m][:] = LayerNorm(x32[m][:], eps) * ln_w + ln_b with the weights of the row's segment.  N in {256,
   512, 1024}; the 352-row tile, whose N / 256 column tiles exchange their partial statistics through memory. */
int32_t me_op_linear_residual_layernorm(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1,
                                        int32_t seg2, const void* const W16[3], const float* const bias[3],
                                        const float* const gamma[3], const float* const ln_w[3], const float* const ln_b[3],
                                        float eps, float* x32, void* xn16);
/* The same launch with the normalised rows written as the next GEMM's MX fp8 operand instead of 16-bit: xn8 [M][N] e4m3
   bytes and xn_scale, one e8m0 byte per 32 columns in the activation layout of me_op_layernorm_fp8 (ceil(M / 128) tiles
   of 128 rows) -- what an ME_DTYPE_FP8 context's 16-bit projection hands to fc1. */
int32_t me_op_linear_residual_layernorm_fp8(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1,
                                            int32_t seg2, const void* const W16[3], const float* const bias[3],
                                            const float* const gamma[3], const float* const ln_w[3], const float* const ln_b[3],
                                            float eps, float* x32, uint8_t* xn8, uint8_t* xn_scale);
/* me_op_linear_fp8 over up to three row segments with their own weights, as the encoder's merged ViT launches run
   it (pipeline.hip MergedVit): rows [0, seg1) use W8[0] / w_scale[0] / bias[0] (/ gamma[0]), [seg1, seg2) the [1]
   set, [seg2, M) the [2] set; seg1, seg2 multiples of 256, seg2 == 0: two segments, seg1 == 0: one. */
int32_t me_op_linear_fp8_segments(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale,
                                  int32_t seg1, int32_t seg2, const uint8_t* const W8[3], const uint8_t* const w_scale[3],
                                  const float* const bias[3], const float* const gamma[3], void* out16, uint8_t* out8,
                                  uint8_t* out8_scale, float* x32);
/* The fp8 GEMM's residual form with the LayerNorm of the rows it updates (csrc/gemm_fp8.hip gemm_pp8t_kernel, the 352-row
   tile): x32[M][N] += gamma * (A8 W8^T + bias) in place and LayerNorm(x32[m][:], eps) * ln_w + ln_b of the row's segment as
   the next GEMM's MX fp8 operand (xn8 / xn_scale as in me_op_linear_residual_layernorm_fp8) -- what an ME_DTYPE_FP8
   context's fc2 hands to the next block's qkv.  Operands as me_op_linear_fp8_segments; N in {256, 512, 1024}. */
int32_t me_op_linear_fp8_residual_layernorm(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale,
                                            int32_t seg1, int32_t seg2, const uint8_t* const W8[3], const uint8_t* const w_scale[3],
                                            const float* const bias[3], const float* const gamma[3], const float* const ln_w[3],
                                            const float* const ln_b[3], float eps, float* x32, uint8_t* xn8, uint8_t* xn_scale);
/* me_op_attention with the output written as an MX fp8 activation operand (out8 [windows*tokens][heads*64] bytes +
   block scales; heads even): the bytes me_op_quantize_fp8 gives for me_op_attention's 16-bit output. */
int32_t me_op_attention_fp8(me_ctx* ctx, const void* qkv16, uint8_t* out8, uint8_t* out8_scale, int32_t windows,
                            int32_t tokens, int32_t heads);
/* me_op_attention (prescaled = 0) / me_op_attention_prescaled (1) over the row space of the encoder's merged ViT launches
   (pipeline.hip MergedVit, gemm_params.h RowSegs): qkv16 [rows_total][3*heads*64]; windows are `tokens` rows apart INSIDE a
   segment -- windows [0, win0) start at row 0, [win0, win0 + win1) at seg1, the rest at seg2 (seg2 == 0: two segments, and
   windows == win0 + win1; seg1 == 0: none, the windows back to back from row 0).  ONE of out16 [rows_total][heads*64] and
   out8 [rows_total][heads*64] e4m3 bytes + out8_scale, one e8m0 byte per 32 columns in the activation layout with
   ceil(rows_total / 128) tiles of 128 rows (heads even) -- what an ME_DTYPE_FP8 context's attention hands to the
   projection.  Rows that belong to no window are neither read nor written.  Refused before any launch: a null pointer,
   both or neither output, an odd head count with out8, segment starts out of order (ME_ERR_BAD_ARG); windows that do
   not fit their segment -- win0 * tokens > seg1, the middle segment's reaching past seg2 (rows_total without a third), the
   last segment's past rows_total (ME_ERR_BAD_SHAPE). */
int32_t me_op_attention_segments(me_ctx* ctx, const void* qkv16, void* out16, uint8_t* out8, uint8_t* out8_scale,
                                 int32_t windows, int32_t tokens, int32_t heads, int32_t prescaled, int64_t rows_total,
                                 int64_t seg1, int64_t seg2, int32_t win0, int32_t win1);
/* me_op_layernorm / me_op_layernorm_fp8 over up to three row segments with their own weights, as the merged ViT launches
   run them: rows [0, seg1) use weight[0] / bias[0], [seg1, seg2) the [1] set, [seg2, rows) the [2] set; seg2 == 0: two
   segments, seg1 == 0: one.  The boundaries may be any rows (the kernels choose per row).  ONE output form: y16 and/or
   y32 [rows][dim] (dim in {64, 128, 256, 512, 1024}), or y8 + yscale as me_op_layernorm_fp8 writes them (dim in {256, 512,
   1024}).  Refused before any launch: a null pointer or a segment without weights, both or neither output form, segment
   starts out of order or beyond `rows` (ME_ERR_BAD_ARG); a dim outside the set (ME_ERR_BAD_SHAPE). */
int32_t me_op_layernorm_segments(me_ctx* ctx, const float* x32, const float* const weight[3], const float* const bias[3],
                                 int64_t seg1, int64_t seg2, void* y16, float* y32, uint8_t* y8, uint8_t* yscale,
                                 int64_t rows, int32_t dim, float eps);
/* The number formatter of the device OBJ writer (csrc/ryu_f64.h, obj_format.hip) on its own: values[i] (DEVICE f64)
   printed as Rust's `{}` prints an f64 -- shortest round-trip digits, positional notation -- into the `stride`-byte
   slot i of `text` (stride >= 344), its length into lengths[i]. */
int32_t me_op_format_f64(me_ctx* ctx, const double* values, int64_t count, char* text, int32_t stride, int32_t* lengths);
/* The record packing of the device PLY writer (csrc/ply_format.h, ply_format.hip) on its own: xyz [nverts][3] and
   faces [nfaces][3] (vertex ids) as the binary records of me_mesh_ply_bytes, from out + header_bytes on: nverts vertex
   records of 24 bytes, or 27 with vertex_rgb [nverts][3], then nfaces face records of 13.  Host or device pointers. */
int32_t me_op_ply_pack(me_ctx* ctx, const float* xyz, const uint8_t* vertex_rgb /* per vertex id, or NULL */,
                       int64_t nverts, const int32_t* faces, int64_t nfaces, int64_t header_bytes,
                       uint8_t* out /* header_bytes + nverts*(24|27) + nfaces*13; the first header_bytes untouched */);
/* The prefix sums of the byte-stream producers (csrc/scan.h) on their own: offsets[i] = base + the sum of counts[0 .. i),
   offsets[n] = base + the total, in 64 bits.  form 0: the one-workgroup scan of the OBJ text (n >= 0); form 1: the
   two-level scan of the JPEG encoder (n > 0).  Host or device pointers. */
int32_t me_op_exclusive_scan_u32(me_ctx* ctx, const uint32_t* counts, int64_t n, uint64_t base, int32_t form,
                                 uint64_t* offsets /* n + 1 */);
/* Box calibration (csrc/calibrate.hip; bench.py's `calibration` object): two FIXED loops on the context's stream, about
   50 ms, synchronous.  out[0] = TFLOP/s of an MFMA-only loop (v_mfma_f32_16x16x32_f16, operands in registers, two waves per
   SIMD on 256 workgroups), out[1] = the shader clock the part held inside it (GHz, s_memtime / s_memrealtime),
   out[2] = GB/s (read + written) of a 512 MiB device copy, out[3] = the loop's ms, out[4] = ms per copy, out[5] = CUs. */
int32_t me_calibrate(me_ctx* ctx, double* out6);
/* f32 <-> context 16-bit type */
int32_t me_op_cast_to16(me_ctx* ctx, const float* src, void* dst16, int64_t count);
int32_t me_op_cast_to32(me_ctx* ctx, const void* src16, float* dst, int64_t count);
/* Per-kernel timing with HIP events on the launch stream (bench.py's roofline leg): enable(1)
   clears and starts recording, report() synchronises and writes a JSON array of
   {"kernel", "launches", "total_ms", "flops", "bytes"} (algorithmic work, summed over launches). */
int32_t me_profile_enable(me_ctx* ctx, int32_t on);
int32_t me_profile_report(me_ctx* ctx, char* json, int64_t capacity);
/* Read-only, a diagnostic counter in the manner of matrix_eyes_hip.h's me_graph_launch_count (kept in this header: the
   integration binding does not need it): how many me_extract_depth[_u8] steps this context has enqueued -- eagerly or
   into a capture -- with the side branch forked (ME_OVERLAP_TAIL=1, csrc/api.hip extract_depth_impl: decoder levels 4 - 2
   and the FOV tail on a second stream, joined in front of level 1).  A replay of a captured step enqueues nothing and
   does not count; 0 for ever when the switch is unset, a progress callback is installed or me_profile_enable is on. */
int64_t me_side_branch_count(const me_ctx* ctx);
/* The per-axis table of image 0.25.10 imageops/sample.rs (vertical_sample / horizontal_sample with the Lanczos3
   kernel) that me_resize_lanczos3_rgb8 runs on: for each output index o of an axis resampled from len_in to len_out
   samples, left[o], count[o] and, packed one index after the other in `weights`, its count[o] normalised weights
   (taps left[o] .. left[o] + count[o] - 1).  Returns the number of weights; when weights_cap is smaller, the number
   needed, writing nothing; < 0 on bad arguments (a length outside [1, ME_RESIZE_MAX_DIM], a null array).
   Unlike the rest of this header it has no context and works on HOST arrays only (the table is built on the host,
   with libm's sinf, whatever the device): it can be tested on a machine without a GPU. */
int64_t me_op_lanczos3_table(int32_t len_in, int32_t len_out, int32_t* left, int32_t* count,
                             float* weights, int64_t weights_cap);
/* The C++ host layer's JPEG decoder (host/jpeg_decoder.cpp decode_jpeg, no orientation) from inside the library: the
   yardstick me_jpeg_decode_rgb8 is measured against in the same process (tools/bench_jpeg.py).  HOST arrays only, no
   context, no GPU; rgb [h,w,3].  0, or < 0 on a null pointer, a size that does not match or a file the decoder refuses. */
int32_t me_op_jpeg_decode_host(const uint8_t* file, int64_t nbytes, uint8_t* rgb, int32_t w, int32_t h);
/* The C++ host layer's PNG decoder (host/png_decoder.cpp decode_png, no orientation) from inside the library: the
   yardstick me_png_decode_rgb8 is measured against in the same process (tools/bench_png_decode.py).  HOST arrays only, no
   context, no GPU; rgb [h,w,3].  0, or < 0 on a null pointer (-1), a size that does not match (-2) or a file the decoder
   refuses (-3: its message is me_last_error(NULL)). */
int32_t me_op_png_decode_host(const uint8_t* file, int64_t nbytes, uint8_t* rgb, int32_t w, int32_t h);
/* The unfilter leg of me_png_decode_rgb8 alone: `stream` is the filtered stream of a picture of the given IHDR fields
   (filter byte plus row, pass after pass: what zlib inflates the IDAT data to), nbytes its length; `out` receives the
   reconstructed stream in the same layout (filter bytes kept).  Host or device pointers, out == stream allowed for device
   memory.  band_rows: picture rows per launch (0: the default; a small value makes a small picture span many launches).
   A host stream with a filter byte above 4 is ME_ERR_BAD_ARG ("bad PNG filter"); in device memory such a row is taken as
   filter 0.  A length that does not match the fields is ME_ERR_BAD_SHAPE. */
int32_t me_op_png_unfilter(me_ctx* ctx, const uint8_t* stream, int64_t nbytes, int32_t width, int32_t height,
                           int32_t bit_depth, int32_t colour_type, int32_t interlace, int32_t band_rows, uint8_t* out);
/* The quantised DCT coefficients of a JPEG file as the host decoder makes them (decode_jpeg_coefficients): all components
   one after the other, natural order, `count` int16_t in all (the layout jpeg_idct_kernel reads).  HOST arrays only, no
   context, no GPU.  0, or < 0 on a null pointer (-1), a count that does not match (-2) or a file the decoder refuses (-3). */
int32_t me_op_jpeg_coefficients_host(const uint8_t* file, int64_t nbytes, int16_t* coef, int64_t count);
/* The same coefficients from the device entropy decoder (csrc/jpeg_entropy.hip) on its own, whatever
   me_ctx_set_jpeg_entropy says; coef a host or device pointer.  subseq_bits: bits per subsequence, a multiple of 32 in
   [64, 65536], 0 for the default (1024): small values make small pictures span many subsequences and workgroups.  A file
   the device decoder declines returns ME_OP_JPEG_ENTROPY_DECLINED (me_last_jpeg_entropy says why) and writes nothing:
   there is no fallback inside this call. */
#define ME_OP_JPEG_ENTROPY_DECLINED 100
int32_t me_op_jpeg_entropy(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t subseq_bits, int16_t* coef,
                           int64_t count);
/* The C++ host layer's JPEG encoder (host/jpeg_encoder.cpp encode_jpeg) from inside the library: the yardstick
   me_jpeg_encode_rgb8 is measured against in the same process.  HOST arrays only, no context, no GPU; rgb [h,w,3], the file
   into jpg[0 .. capacity), its size into *nbytes.  0, or < 0 on a null pointer (-1), parameters the encoder refuses (-2) or
   a capacity that is too small (-3: *nbytes says what is needed, nothing is written). */
int32_t me_op_jpeg_encode_host(const uint8_t* rgb, int32_t w, int32_t h, int32_t quality, int32_t subsampling,
                               uint8_t* jpg, int64_t capacity, int64_t* nbytes);
/* The context's last JPEG encode.  report: [0] blocks of the scan (dummy blocks included), [1] bits of the scan before the
   padding, [2] stuffed 00 bytes, [3] bytes of the file, workgroups of [4] jpeg_fdct_kernel, [5] jpeg_bits_kernel and
   jpeg_pack_kernel, [6] the scan over the blocks' bit counts, [7] the two stuffing kernels, [8] the scan over their counts,
   [9] bytes of the file buffer the encode was sized for (header + twice the packed stream + 2).  ms, HIP event times:
   [0] upload of a host picture and the tables, [1] fdct, [2] bits and their scan, [3] pack (with the read-back of the
   scan's bits), [4] stuffing, [5] download of the file (0 when it stayed on the device). */
int32_t me_last_jpeg_encode(me_ctx* ctx, int64_t report[10], double ms[6]);
/* One pack kernel of the device weight packer (csrc/weight_pack.hip) on its own: a tensor of `dims` in the checkpoint's
   layout and element type src_dtype (ME_WEIGHT_*) into the arena layout of `kind` -- 0 flat f32, 1 16-bit matrix
   [N][K], 2 Conv2d [Cout][Cin][kh][kw] -> [Cout][kh*kw][Cin], 3 ConvTranspose2d [Cin][Cout][2][2] -> [(dy*2+dx)*Cout + co][Cin],
   4 [1][Cin][k][k] -> f32 [k][k][Cin] -- in the context's 16-bit type, with every run of K (or Cin) values written twice,
   [W | W], when dup != 0 (kinds 1 - 3).  dst receives numel * (dup ? 2 : 1) elements.  Host or device pointers.  Dimensions
   that do not fit the kind (or more than 64 taps) are ME_ERR_BAD_SHAPE. */
int32_t me_op_weight_pack(me_ctx* ctx, int32_t kind, int32_t dup, const int64_t* dims, int32_t ndim, const void* src,
                          int32_t src_dtype, void* dst);
/* The host packer (csrc/weight_pack.h pack_host, the loops me_load_weight runs with packer 0) without a context: dtype is
   ME_DTYPE_F16 or ME_DTYPE_BF16.  HOST arrays only, no GPU.  0, or < 0 on a null pointer (-1), a bad dtype (-2) or
   dimensions that do not fit the kind (-3). */
int32_t me_op_weight_pack_host(int32_t dtype, int32_t kind, int32_t dup, const int64_t* dims, int32_t ndim, const void* src,
                               int32_t src_dtype, void* dst);
/* The legacy stereogram noise of the C++ host layer (host/matrix_eyes.cpp DepthMap::output_stereogram: std::mt19937(seed),
   four little-endian bytes per draw) into out [nbytes]: the same loop compiled into the library, so that
   tools/bench_stereogram_noise.py can time it in one process beside the keyed noise.  HOST memory, no GPU, no context; a
   null pointer or a negative size is ME_ERR_BAD_ARG. */
int32_t me_op_legacy_noise_host(uint32_t seed, int64_t nbytes, uint8_t* out);
/* Names of the GEMM tile configurations (for reports). */
int32_t me_op_gemm_config_count(void);
const char* me_op_gemm_config_name(int32_t cfg);

#ifdef __cplusplus
}
#endif
#endif /* MATRIX_EYES_HIP_OPS_H */
