// The launch descriptors (common.h GemmParams) of every GEMM, convolution and ConvTranspose form the model runs: host code,
// shared by the forward pass (pipeline.hip) and the kernel-level entries (api.hip me_op_*), so that the op tests launch what
// the pipeline launches.  A builder takes operands and shapes and fills what the kernels read; which tile runs, split-K,
// grid_cap and the profiler's flop_rows stay with the caller.
#pragma once
#include "model.h"

namespace me {

// the one place a GemmParams is value-initialised: every pointer null, every int 0, no clamp
inline GemmParams base_params() {
    GemmParams p = GemmParams();
    p.clamp_lo = -INFINITY, p.clamp_hi = INFINITY;
    return p;
}

// out = act(A[M][K] . W[N][K]^T + bias) as 16-bit and/or f32 rows of N
inline GemmParams linear_params(int64_t M, int N, int K, const void* A, const void* W, const float* bias, void* out16,
                                float* out32, int act = ACT_NONE) {
    GemmParams p = base_params();
    p.M = (int)M, p.N = N, p.K = K, p.A = A, p.lda = K, p.W = W, p.bias = bias;
    p.out16 = out16, p.out32 = out32, p.ldc = N, p.act = act;
    return p;
}
// Split operands (model.h SplitStage).  The A rows hold `parts` K-wide parts ([hi | lo], [hi | lo | hi]) against weights
// stored [W | W (| W)]: the kernel walks parts * K, the layer's FLOPs stay those of K
// wrap_third ([hi | lo | hi] only): the rows are stored two parts wide and the kernel reads the third part from the first
// (GemmParams::a_wrap) -- the same K order against the same weights, a third of the operand's bytes neither written nor read
inline void set_a_wrap(GemmParams& p, int stored_k) { p.lda = stored_k, p.a_wrap = stored_k / 64; }
inline void set_a_parts(GemmParams& p, int parts, bool wrap_third = false) {
    const int part_k = p.K;
    p.flop_k = part_k, p.K *= parts, p.lda = p.K;
    if (parts == 3 && wrap_third) set_a_wrap(p, 2 * part_k);
}
// ... and the 16-bit output is written as rows / pixels of `parts` C-wide parts
inline void set_out16_parts(GemmParams& p, int64_t C, int parts) {
    if (parts >= 2) p.ldc16 = parts * C, p.lo_off16 = (int32_t)C;
    if (parts == 3) p.hi2_off16 = (int32_t)(2 * C);
}
// the qkv linear: columns n < qcols (Q) leave scaled for the attention kernel
inline void set_scaled_cols(GemmParams& p, int qcols, float qscale) { p.qcols = qcols, p.qscale = qscale; }
// out16 is a zero-bordered NHWC map [B][H+2][W+2][N] of the M = B * H * W rows
inline void set_out16_bordered(GemmParams& p, int H, int W) { p.out16_border = 1, p.out_H = H, p.out_W = W; }

// EPI_RESID_SCALE: x += gamma * (A W^T + bias), in place
inline GemmParams resid_params(int64_t M, int N, int K, const void* A, const void* W, const float* bias, const float* gamma,
                               float* x32) {
    GemmParams p = linear_params(M, N, K, A, W, bias, nullptr, x32);
    p.gamma = gamma, p.res32 = x32;
    return p;
}

// EPI_PATCH_EMBED (vit.rs:287-295): `windows` x P patches of 768 values -> token rows 1.. of each window, + pos
inline GemmParams patch_embed_params(int windows, int P, int C, const void* patches16, const void* W, const float* bias,
                                     const float* pos, float* tokens32) {
    GemmParams p = linear_params((int64_t)windows * P, C, 768, patches16, W, bias, nullptr, tokens32);
    p.pos = pos, p.tokens_per_window = P;
    return p;
}

struct ConvOut {
    float* out32 = nullptr;   // [B*H*W][Cout]
    void* out16 = nullptr;    // 16-bit copy
    bool border16 = false;    // out16 is [B][H+2][W+2][Cout]
    int parts16 = 1;          // out16 pixels are [hi | lo] of 2*Cout (2) or [hi | lo | hi] of 3*Cout (3)
    int act = ACT_NONE;       // applied to out16 (and out32 unless act16_only)
    bool act16_only = true;
    const float* res32 = nullptr;
    const float* res32b = nullptr;
    const float* tap_bias = nullptr;  // GemmParams::tap_bias ([9][Cout]; needs border16)
};

// the A_CONV operand: a zero-bordered NHWC map [B][Hin+2][Win+2][Cin], k x k taps (k = 1 or 3, pad (k-1)/2, stride 1 or 2)
// a_split: pixels of [hi | lo]; the packed weights repeat each tap's Cin values
inline GemmParams conv_operand(const void* in16b, int B, int Hin, int Win, int Cin, const void* W, int N, int k, int stride,
                               const float* bias, bool a_split) {
    GemmParams p = base_params();
    p.flop_k = k * k * Cin;
    if (a_split) Cin *= 2;
    p.out_H = Hin / stride, p.out_W = Win / stride;
    p.M = B * p.out_H * p.out_W, p.N = N, p.K = k * k * Cin;
    p.A = in16b, p.in_Hp = Hin + 2, p.in_Wp = Win + 2, p.Cin = Cin, p.KH = k, p.KW = k, p.stride = stride;
    p.W = W, p.bias = bias;
    return p;
}
// Conv2d k x k on a zero-bordered NHWC operand (EPI_STORE)
inline GemmParams conv_params(const void* in16b, int B, int Hin, int Win, int Cin, const void* W, int Cout, int k, int stride,
                              const float* bias, const ConvOut& o, bool a_split = false) {
    GemmParams p = conv_operand(in16b, B, Hin, Win, Cin, W, Cout, k, stride, bias, a_split);
    p.res32 = o.res32, p.res32b = o.res32b, p.tap_bias = o.tap_bias;
    p.out32 = o.out32, p.out16 = o.out16, p.ldc = Cout, p.out16_border = o.border16 ? 1 : 0;
    p.act = o.act, p.act16_only = o.act16_only ? 1 : 0;
    set_out16_parts(p, Cout, o.parts16);
    return p;
}

// ConvTranspose2d(2,2,stride 2) of an unbordered NHWC operand [B*H*W][Cin] -> [B][2H][2W][Cout] (EPI_CONVT)
// pixel_stride: channels per pixel of out16 when it is a slice of a wider map (0: Cout, or 2 Cout when split);
// out_split: out16 pixels are [hi | lo], the lo part lo_off channels after the hi part (0: Cout);
// k_copies > 0: A rows hold this many Cin-wide parts ([hi | lo | hi] = 3; wrap_third: stored [hi | lo], set_a_parts)
inline GemmParams convt_params(const void* in16, int B, int H, int W_, int Cin, const void* W, int Cout, const float* bias,
                               float* out32, void* out16, bool border16, int64_t pixel_stride, int act16, bool a_split = false,
                               bool out_split = false, int64_t lo_off = 0, int k_copies = 0, bool wrap_third = false) {
    GemmParams p = linear_params((int64_t)B * H * W_, 4 * Cout, Cin, in16, W, bias, out16, out32, act16);
    set_a_parts(p, k_copies > 0 ? k_copies : (a_split ? 2 : 1), wrap_third);
    // the composed deconv o out_conv (k_copies == 3) stands for two layers of SURVEY App. B: ConvT (Cin x 4 Cout per
    // input pixel) and the 1x1 conv at 4x the pixels (Cout x Cout each) -- twice the ConvT's FLOPs when Cin == Cout
    if (k_copies == 3) p.flop_k = 2 * Cin;
    p.out_H = H, p.out_W = W_, p.Cout = Cout, p.out16_border = border16 ? 1 : 0, p.ldc = Cout;
    if (out_split) p.lo_off16 = (int32_t)(lo_off ? lo_off : Cout);
    if (out_split || pixel_stride) p.ldc16 = pixel_stride ? pixel_stride : 2 * Cout;
    return p;
}

// Two ConvTransposes over the SAME input grid onto the same [B][2H][2W][Cout] map as one launch (GemmParams::A2; the 256x256
// two-group tile): `first` (no bias) keeps its 16-bit output (activation, border) and gives up its f32 one, `second` gives the
// launch its operands as the chained set; out32 = (sum over K of first + sum over K of second) + second's bias, summed in one
// accumulator.
inline GemmParams chain_convt(const GemmParams& first, const GemmParams& second, float* out32) {
    GemmParams p = first;
    p.out32 = out32;
    p.A2 = second.A, p.W2 = second.W, p.lda2 = second.lda, p.K2 = second.K, p.a_wrap2 = second.a_wrap, p.bias2 = second.bias;
    p.flop_k2 = second.flop_k ? second.flop_k : second.K;
    return p;
}

// EPI_HEAD_FINAL (mod.rs:330-333, :361-362): conv3x3 (Cin -> Cmid <= 32) + ReLU + conv1x1 (w2, b2) + ReLU, / f_norm, clamp
inline GemmParams head_final_params(const void* in16b, int B, int H, int W_, int Cin, const void* W, int Cmid, const float* bias,
                                    const float* w2, const float* b2, const float* f_norm, float clamp_lo, float clamp_hi,
                                    float* out32, bool a_split = false) {
    GemmParams p = conv_operand(in16b, B, H, W_, Cin, W, Cmid, 3, 1, bias, a_split);
    p.w2 = w2, p.b2 = b2, p.f_norm = f_norm, p.pixels_per_image = H * W_, p.out32 = out32;
    p.clamp_lo = clamp_lo, p.clamp_hi = clamp_hi;
    return p;
}
// EPI_HEAD_COMPOSED (head_composed_launch): the same behind the composed ConvTranspose o conv3x3 on the half-resolution map
// [B][H][W]: 4 output phases x 32 channels, tap_bias [9][32], out32 the full-resolution depth [B][2H][2W]
inline GemmParams head_composed_params(const void* in16b, int B, int H, int W_, int Cin, const void* W, const float* bias,
                                       const float* tap_bias, const float* w2, const float* b2, const float* f_norm,
                                       float clamp_lo, float clamp_hi, float* out32) {
    GemmParams p = head_final_params(in16b, B, H, W_, Cin, W, 128, bias, w2, b2, f_norm, clamp_lo, clamp_hi, out32);
    p.tap_bias = tap_bias, p.pixels_per_image = 4 * H * W_;
    return p;
}

// Row segments with their own weights (GemmParams::seg1 / seg2): set i belongs to segment i
struct SegWeights {
    const void* W[3] = {};
    const float *bias[3] = {}, *gamma[3] = {};
    const uint8_t* w_scale[3] = {};  // MX fp8 weights
};
// from the arrays of three the op entries take (w_scale, gamma: may be null)
template <class Wt>
inline SegWeights seg_weights(const Wt* const W[3], const uint8_t* const w_scale[3], const float* const bias[3], const float* const gamma[3]) {
    SegWeights s;
    for (int i = 0; i < 3; ++i)
        s.W[i] = W[i], s.bias[i] = bias[i], s.gamma[i] = gamma ? gamma[i] : nullptr, s.w_scale[i] = w_scale ? w_scale[i] : nullptr;
    return s;
}
inline void set_segments(GemmParams& p, int64_t seg1, int64_t seg2, const SegWeights& w) {
    p.seg1 = (int)seg1, p.seg2 = (int)seg2;
    p.W = w.W[0], p.bias = w.bias[0], p.gamma = w.gamma[0], p.w_scale = w.w_scale[0];
    p.W_s1 = w.W[1], p.bias_s1 = w.bias[1], p.gamma_s1 = w.gamma[1], p.w_scale_s1 = w.w_scale[1];
    p.W_s2 = w.W[2], p.bias_s2 = w.bias[2], p.gamma_s2 = w.gamma[2], p.w_scale_s2 = w.w_scale[2];
}

// MX fp8 (gemm_fp8_launch): A and W are e4m3 bytes with e8m0 block scales (mx_fp8.h; the A scales in 128-row tiles) ...
inline void set_fp8_operands(GemmParams& p, const uint8_t* a_scale, const uint8_t* w_scale) {
    p.a_scale = a_scale, p.a_mt = (int)cdiv((int64_t)p.M, 128), p.w_scale = w_scale;
}
// ... and the output leaves as the next GEMM's fp8 operand
inline void set_out8(GemmParams& p, uint8_t* out8, uint8_t* out8_scale) {
    p.out8 = out8, p.out8_scale = out8_scale, p.out8_mt = (int)cdiv((int64_t)p.M, 128);
}

// LayerNorm weights of the three row segments for a launch that normalises the rows it updates
struct LnSet {
    const float *w0 = nullptr, *b0 = nullptr, *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
};
// The residual update and the LayerNorm behind it in one launch (gemm_core.h resid_ln_epilogue; p: resid_params with its
// segments set, for the 352-row tile): the normalised rows leave as 16-bit xn16, or as MX fp8 xn8 + xn_scale.  The column
// tiles of a row tile exchange their partial statistics through two scratch buffers of the context, sized HERE and nowhere
// else: ln_stats [row tile][N / 256][352] granules of 8 bytes, ln_count one word per row tile, 64 bytes apart (zero when
// allocated, never reset: it advances by N / 256 per launch, so launches of different N must not share one -- count_site).
inline void set_fused_layernorm(me_ctx* ctx, GemmParams& p, const std::string& stats_site, const std::string& count_site,
                                const LnSet& ln, float eps, void* xn16, uint8_t* xn8, uint8_t* xn_scale) {
    p.ln_out16 = xn8 ? (void*)xn8 : xn16, p.ln_eps = eps;  // (ln_out16 != null is the kernels' switch, fp8 or not)
    if (xn8) set_out8(p, xn8, xn_scale);
    p.ln_w = ln.w0, p.ln_b = ln.b0, p.ln_w_s1 = ln.w1, p.ln_b_s1 = ln.b1, p.ln_w_s2 = ln.w2, p.ln_b_s2 = ln.b2;
    const size_t row_tiles = (size_t)seg_row_tiles<352>(p.M, p.seg1, p.seg2);
    p.ln_stats = (unsigned long long*)site_buf(ctx, stats_site, row_tiles * (size_t)(p.N / 256) * 352 * 8);
    p.ln_count = (unsigned*)site_buf(ctx, count_site, row_tiles * 64);
}

}  // namespace me
