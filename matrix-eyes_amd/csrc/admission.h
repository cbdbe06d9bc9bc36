// What a launcher or a kernel-level entry refuses before anything is launched: the shape, stride, count and boundary rules of
// gemm_launch (gemm.hip), gemm_fp8_launch (gemm_fp8.hip), attention_launch (attention.hip) and the me_op_* entries (api.hip) as pure
// functions of the descriptor.  The kernels trust their descriptors -- a caller mistake past these lines is a device fault, not a
// status code --, so the rules live where a host compiler and a sanitizer can hold them: free of HIP, of the context and of getenv
// (tests/test_admission_cpu.py, against the answers the checks gave where they stood before this header existed).  Each function
// raises through ME_CHECK, in the order its launcher always checked.  Which TILE takes a problem is tile_choice.h's
// (config_refusal); the K >= 128 checks of the launch templates stay in gemm_core.h.  DESIGN.md 4.45.
#pragma once
#include "gemm_params.h"

namespace me {

// ---- shared rules ---------------------------------------------------------------------------------------
// Row segments [0, seg1), [seg1, seg2), [seg2, rows): both starts inside the rows, the second only behind a first
inline bool row_segments_ordered(int64_t seg1, int64_t seg2, int64_t rows) {
    return seg1 >= 0 && seg2 >= 0 && seg1 <= rows && seg2 <= rows && (seg2 == 0 || (seg1 > 0 && seg2 > seg1));
}
inline void admit_row_segments(const char* who, int64_t seg1, int64_t seg2, int64_t rows) {
    ME_CHECK(row_segments_ordered(seg1, seg2, rows), ME_ERR_BAD_ARG, "%s: segments %lld / %lld of %lld rows", who, (long long)seg1,
             (long long)seg2, (long long)rows);
}
inline int row_segment_count(int64_t seg1, int64_t seg2) { return seg1 == 0 ? 1 : (seg2 == 0 ? 2 : 3); }
// every array of three pointers (one per segment) has one for each segment the launch has
template <class... P>
inline void admit_segment_weights(const char* who, int64_t seg1, int64_t seg2, const P* const*... arrays) {
    const int nseg = row_segment_count(seg1, seg2);
    for (int i = 0; i < nseg; ++i) ME_CHECK((... && (arrays[i] != nullptr)), ME_ERR_BAD_ARG, "%s: row segment %d without weights", who, i);
}

// The LayerNorm of the updated rows inside the residual epilogue (GemmParams::ln_out16), as both GEMM launchers take it.
// prefix: "gemm" / "fp8 gemm".  resid_operands: the 16-bit launcher asks for the residual form's own operands here, in this clause;
// the fp8 launcher has refused their absence earlier, with its own message.
inline void admit_fused_layernorm(const char* prefix, const GemmParams& p, bool resid_operands) {
    ME_CHECK((p.N == 256 || p.N == 512 || p.N == 1024) && p.ldc == p.N && p.ln_w && p.ln_b && p.ln_stats && p.ln_count &&
                 (!resid_operands || (p.bias && p.gamma && p.res32 && p.out32)),
             ME_ERR_BAD_ARG, "%s: the fused LayerNorm takes N in {256, 512, 1024} with its weights, statistics and counters", prefix);
    ME_CHECK(p.seg1 == 0 || (p.ln_w_s1 && p.ln_b_s1 && (p.seg2 == 0 || (p.ln_w_s2 && p.ln_b_s2))), ME_ERR_BAD_ARG,
             "%s: a row segment without LayerNorm weights", prefix);
    // out8 beside ln_out16: the normalised rows leave as MX fp8 + activation-layout scales instead of 16-bit
    if (p.out8)
        ME_CHECK(p.out8_scale && (int64_t)p.out8_mt * 128 >= p.M, ME_ERR_BAD_ARG,
                 "%s: the fused LayerNorm's fp8 output needs its block scales (%d tiles of 128 rows for %d rows)", prefix, p.out8_mt, p.M);
}

// ---- gemm_launch (16-bit operands) ----------------------------------------------------------------------
// A difference from admit_gemm_fp8 that is kept: this launcher does NOT test the weights, biases and gammas of row segments 1 and 2
// for null, nor the segment starts against M (config_refusal holds them to the tile's boundaries and their order); its entries do
// (admit_op_linear_segments below; the pipeline builds its own descriptors).
inline void admit_gemm(const GemmParams& p, AMode amode, EpiKind epi) {
    ME_CHECK(p.M > 0 && p.N > 0 && p.K > 0, ME_ERR_BAD_SHAPE, "gemm: empty problem %dx%dx%d", p.M,
             p.N, p.K);
    ME_CHECK(p.K % 64 == 0, ME_ERR_BAD_SHAPE, "gemm: K=%d is not a multiple of 64", p.K);
    ME_CHECK(p.M < (1 << 30) && p.N < (1 << 30), ME_ERR_BAD_SHAPE, "gemm: %dx%d too large", p.M, p.N);
    ME_CHECK(p.N % 4 == 0, ME_ERR_BAD_SHAPE, "gemm: N=%d is not a multiple of 4", p.N);
    ME_CHECK(p.A && p.W, ME_ERR_BAD_ARG, "gemm: null operand");
    if (amode == A_CONV) {
        ME_CHECK(p.Cin % 64 == 0 && p.K == p.KH * p.KW * p.Cin, ME_ERR_BAD_SHAPE,
                 "conv: Cin=%d K=%d KHxKW=%dx%d", p.Cin, p.K, p.KH, p.KW);
        ME_CHECK(p.out_H > 0 && p.out_W > 0 && p.M % (p.out_H * p.out_W) == 0, ME_ERR_BAD_SHAPE,
                 "conv: M=%d is not a multiple of %dx%d", p.M, p.out_H, p.out_W);
    } else {
        // (a_wrap: the row ends where the wrapped slabs start over)
        ME_CHECK(p.a_wrap >= 0 && p.a_wrap < p.K / 64 && (p.a_wrap == 0 || (epi == EPI_CONVT && p.K - p.a_wrap * 64 <= p.a_wrap * 64)),
                 ME_ERR_BAD_ARG, "gemm: a_wrap=%d of %d slabs", p.a_wrap, p.K / 64);
        ME_CHECK(p.lda % 8 == 0 && p.lda >= (p.a_wrap ? p.a_wrap * 64 : p.K), ME_ERR_BAD_SHAPE, "gemm: lda=%lld K=%d",
                 (long long)p.lda, p.K);
    }
    if (p.A2) {
        // a chained operand set: what the kernel's two passes assume (which tile: tile_choice.h config_refusal)
        ME_CHECK(p.W2 && p.out16 && p.out32 && !p.bias && !p.lo_off16 && p.seg1 == 0 && p.act != ACT_GELU, ME_ERR_BAD_ARG,
                 "gemm: a chained operand set takes an unbiased first set with a plain 16-bit output, and an f32 output");
        ME_CHECK(p.K2 > 0 && p.K2 % 64 == 0 && p.a_wrap2 >= 0 && p.a_wrap2 < p.K2 / 64 &&
                     (p.a_wrap2 == 0 || p.K2 - p.a_wrap2 * 64 <= p.a_wrap2 * 64) && p.lda2 % 8 == 0 &&
                     p.lda2 >= (p.a_wrap2 ? p.a_wrap2 * 64 : p.K2),
                 ME_ERR_BAD_SHAPE, "gemm: chained operand set K=%d lda=%lld a_wrap=%d", p.K2, (long long)p.lda2, p.a_wrap2);
    }
    // The ConvTranspose epilogue places an 8-column granule by the sub-pixel and channel of its first column (gemm_core.h EpiLane
    // q / co).  With Cout = 8 k + 4 every other sub-pixel boundary falls inside a granule: the run-time epilogue mode places such a
    // granule's halves separately (tests/test_gpu_redzone.py found the unsplit granule: bias read from behind the vector, four
    // channels in the neighbouring pixel, the sub-pixel's first four never written).  The chained launch has compiled-in modes
    // only and keeps whole granules; a half-granule (four columns, the unit of every store here) may not straddle anything.
    if (epi == EPI_CONVT) {
        ME_CHECK(p.Cout > 0 && p.Cout % 4 == 0, ME_ERR_BAD_SHAPE, "convt: Cout=%d is not a multiple of 4", p.Cout);
        ME_CHECK(!p.A2 || p.Cout % 8 == 0, ME_ERR_BAD_SHAPE, "convt: a chained launch takes Cout in multiples of 8, not %d", p.Cout);
    }
    if (epi == EPI_HEAD_FINAL) ME_CHECK(p.N <= 32, ME_ERR_BAD_SHAPE, "head: N=%d > 32", p.N);
    if (p.tap_bias)  // the epilogue needs the output pixel's coordinates: the bordered 16-bit output has them
        ME_CHECK(amode == A_CONV && epi == EPI_STORE && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.out16 && p.out16_border && p.bias &&
                     p.N % 8 == 0 && !p.out32 && !p.res32 && !p.res32b && !p.lo_off16 && !p.hi2_off16 && p.act != ACT_GELU,
                 ME_ERR_BAD_ARG, "conv: per-tap bias shares take a 3x3 stride-1 convolution with a bordered 16-bit output and nothing else");
    // (that the fused LayerNorm runs on the 352-row tile's residual epilogue: tile_choice.h config_refusal)
    if (p.ln_out16) admit_fused_layernorm("gemm", p, true);
    if (p.qcols)
        ME_CHECK(epi == EPI_STORE && p.qcols % 64 == 0 && p.qcols <= p.N && p.out16 && !p.out32 && p.act == ACT_NONE &&
                     !p.lo_off16 && !p.hi2_off16,
                 ME_ERR_BAD_ARG, "gemm: scaled leading columns (qcols = %d) take a plain 16-bit output", p.qcols);
}

// the head's composed ConvTranspose o conv3x3 o conv1x1 launch (gemm.hip head_composed_launch): the one shape its halo tile takes
inline bool head_composed_fits(const GemmParams& p) {
    return p.N == 128 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.Cin % 64 == 0 && p.K == 9 * p.Cin && p.out_H % 16 == 0 &&
           p.out_W % 16 == 0 && p.M % 256 == 0 && p.M == (p.M / (p.out_H * p.out_W)) * p.out_H * p.out_W;
}
inline void admit_head_composed(const GemmParams& p) {
    ME_CHECK(head_composed_fits(p), ME_ERR_BAD_SHAPE, "composed head: %dx%d map, Cin %d, N %d", p.out_H, p.out_W, p.Cin, p.N);
    ME_CHECK(p.A && p.W && p.bias && p.tap_bias && p.w2 && p.b2 && p.out32 && p.pixels_per_image == 4 * p.out_H * p.out_W,
             ME_ERR_BAD_ARG, "composed head: missing operand");
}

// ---- gemm_fp8_launch (MX fp8 operands) ------------------------------------------------------------------
// A difference from admit_gemm that is kept: only this launcher tests the segment weights, scales, biases and gammas for null and
// the segment starts against M -- a caller mistake here would be a device fault, not a status code.
inline void admit_gemm_fp8(const GemmParams& p, EpiKind epi) {
    ME_CHECK(p.M > 0 && p.N > 0 && p.N % 256 == 0 && p.K % 128 == 0 && p.K >= 256, ME_ERR_BAD_SHAPE,
             "fp8 gemm: M=%d N=%d K=%d (N a multiple of 256; K a multiple of 128 and >= 256)", p.M, p.N, p.K);
    ME_CHECK(p.A && p.W && p.a_scale && p.w_scale && p.a_mt * 128 >= p.M, ME_ERR_BAD_ARG, "fp8 gemm: operands");
    ME_CHECK(p.lda % 16 == 0 && p.lda >= p.K, ME_ERR_BAD_SHAPE, "fp8 gemm: lda=%lld", (long long)p.lda);
    ME_CHECK(p.seg1 % 16 == 0 && p.seg2 % 16 == 0 && p.seg1 >= 0 && p.seg2 >= 0 && p.seg1 <= p.M && p.seg2 <= p.M, ME_ERR_BAD_ARG,
             "fp8 gemm: row segments %d / %d of %d rows", p.seg1, p.seg2, p.M);
    ME_CHECK(p.seg1 == 0 || (p.W_s1 && p.w_scale_s1), ME_ERR_BAD_ARG, "fp8 gemm: row segment 1 without weights / scales");
    ME_CHECK(p.seg2 == 0 || (p.seg1 != 0 && p.seg2 > p.seg1 && p.W_s2 && p.w_scale_s2), ME_ERR_BAD_ARG,
             "fp8 gemm: row segment 2 without weights / scales");
    if (epi == EPI_RESID_SCALE) {
        ME_CHECK(p.gamma && p.res32 && p.out32 && p.bias, ME_ERR_BAD_ARG, "fp8 gemm: the residual form takes bias, gamma, res32 and out32");
        ME_CHECK((p.seg1 == 0 || (p.gamma_s1 && p.bias_s1)) && (p.seg2 == 0 || (p.gamma_s2 && p.bias_s2)), ME_ERR_BAD_ARG,
                 "fp8 gemm: a row segment without bias / gamma");
    } else {
        ME_CHECK((p.seg1 == 0 || p.bias_s1) && (p.seg2 == 0 || p.bias_s2), ME_ERR_BAD_ARG, "fp8 gemm: a row segment without bias");
    }
    // the residual form with the LayerNorm of the updated rows (GemmParams::ln_out16 / out8 as in gemm_launch)
    if (epi == EPI_RESID_SCALE && (p.ln_out16 || p.out8)) admit_fused_layernorm("fp8 gemm", p, false);
    // the two output forms of the store epilogue, last: a call refused above keeps the message it always had
    if (epi == EPI_STORE) {
        if (p.out8)
            ME_CHECK(p.out8_scale && p.out8_mt * 128 >= p.M && p.bias, ME_ERR_BAD_ARG, "fp8 gemm: fp8 output");
        else
            ME_CHECK(p.out16 && !p.out32 && !p.res32 && p.bias && !p.out16_border, ME_ERR_BAD_ARG,
                     "fp8 gemm: the 16-bit output form takes bias and out16 only");
    }
}

// f16 rows -> e4m3 + e8m0 scales (gemm_fp8.hip quantize_f16_to_fp8_launch): whole MX blocks of 128, weight rows in tiles of 64
inline void admit_quantize_fp8(int64_t rows, int32_t K, int32_t weight_layout) {
    ME_CHECK(K % 128 == 0 && rows > 0, ME_ERR_BAD_SHAPE, "fp8 quantise: rows=%lld K=%d", (long long)rows, K);
    if (weight_layout) ME_CHECK(rows % 64 == 0, ME_ERR_BAD_SHAPE, "fp8 quantise: %lld weight rows", (long long)rows);
}

// ---- attention_launch -----------------------------------------------------------------------------------
inline void admit_attention(int32_t windows, int32_t tokens, int32_t heads, const uint8_t* out8, const uint8_t* out8_scale,
                            int64_t out8_mt) {
    ME_CHECK(windows > 0 && tokens > 0 && heads > 0, ME_ERR_BAD_SHAPE,
             "attention: windows=%d tokens=%d heads=%d", windows, tokens, heads);
    ME_CHECK(!out8 || (out8_scale && out8_mt > 0 && heads % 2 == 0), ME_ERR_BAD_ARG,
             "attention: fp8 output needs its scale buffer and K = 64 heads a multiple of 128");
    ME_CHECK((int64_t)windows * heads * ((tokens + 127) / 128) < (1ll << 30), ME_ERR_BAD_SHAPE,
             "attention: grid too large");
}

// ---- the me_op_* entries (api.hip): GEMM, convolution and ConvTranspose forms ---------------------------
// (the act values are the ABI's ME_ACT_*, which are Act's)
inline void admit_op_conv2d(int32_t k, int32_t stride) {
    ME_CHECK((k == 1 || k == 3) && (stride == 1 || stride == 2), ME_ERR_BAD_SHAPE,
             "me_op_conv2d: k=%d stride=%d", k, stride);
}
inline void admit_op_head_final(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cmid) {
    ME_CHECK(B > 0 && H > 0 && W > 0 && Cin % 64 == 0 && Cmid > 0 && Cmid <= 32 && Cmid % 4 == 0, ME_ERR_BAD_SHAPE,
             "me_op_head_final: %d x %d x %d, %d -> %d", B, H, W, Cin, Cmid);
}
inline void admit_op_conv2d_forms(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, const void* out16,
                                  int32_t out16_parts, int32_t act) {
    ME_CHECK((k == 1 || k == 3) && (stride == 1 || stride == 2) && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 &&
                 H % stride == 0 && W % stride == 0,
             ME_ERR_BAD_SHAPE, "me_op_conv2d_forms: %d x %d x %d, %d -> %d, k=%d stride=%d", B, H, W, Cin, Cout, k, stride);
    ME_CHECK(out16_parts >= 1 && out16_parts <= 3 && (out16_parts == 1 || out16), ME_ERR_BAD_ARG,
             "me_op_conv2d_forms: out16_parts=%d", out16_parts);
    ME_CHECK(act == ACT_NONE || act == ACT_RELU, ME_ERR_BAD_ARG, "me_op_conv2d_forms: act=%d", act);
}
// a_wrap > 0: the operand rows are stored a_wrap channels wide and channels a_wrap .. Cin - 1 are read from the row's start
inline void admit_a_wrap(const char* who, int32_t Cin, int32_t a_wrap) {
    ME_CHECK(a_wrap >= 0 && a_wrap % 64 == 0 && (a_wrap == 0 || (a_wrap < Cin && Cin - a_wrap <= a_wrap)), ME_ERR_BAD_SHAPE,
             "%s: a_wrap=%d of %d channels", who, a_wrap, Cin);
}
inline void admit_op_conv_transpose2x2_forms(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t a_wrap, int32_t Cout, const void* out16,
                                             int32_t act16, int32_t out_split, int32_t pixel_stride, int32_t lo_off) {
    // (Cout = 8 k + 4 runs: the epilogue's run-time mode splits the granules that straddle a sub-pixel; pixel_stride and lo_off
    // stay multiples of 8, so a split output of such a Cout takes both explicitly)
    ME_CHECK(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cout % 4 == 0, ME_ERR_BAD_SHAPE,
             "me_op_conv_transpose2x2_forms: %d x %d x %d, %d -> %d", B, H, W, Cin, Cout);
    ME_CHECK(act16 == ACT_NONE || act16 == ACT_RELU, ME_ERR_BAD_ARG, "me_op_conv_transpose2x2_forms: act16=%d", act16);
    ME_CHECK((!out_split && !pixel_stride && !lo_off) || out16, ME_ERR_BAD_ARG,
             "me_op_conv_transpose2x2_forms: a 16-bit layout without a 16-bit output");
    ME_CHECK(out_split || !lo_off, ME_ERR_BAD_ARG, "me_op_conv_transpose2x2_forms: lo_off without out_split");
    const int lo = out_split ? (lo_off ? lo_off : Cout) : 0;
    ME_CHECK(pixel_stride >= 0 && pixel_stride % 8 == 0 && lo % 8 == 0 && (!out_split || lo >= Cout) &&
                 (!pixel_stride || pixel_stride >= lo + Cout),
             ME_ERR_BAD_SHAPE, "me_op_conv_transpose2x2_forms: pixel_stride=%d lo_off=%d for %d channels", pixel_stride, lo_off, Cout);
    admit_a_wrap("me_op_conv_transpose2x2_forms_wrap", Cin, a_wrap);
}
inline void admit_op_conv_transpose2x2_pair(int32_t B, int32_t H, int32_t W, int32_t Cout, int32_t Cin_a, int32_t Cin_b, int32_t a_wrap_b,
                                            int32_t act16, int32_t grid_cap) {
    ME_CHECK(B > 0 && H > 0 && W > 0 && Cin_a > 0 && Cin_b > 0 && Cout > 0 && Cout % 8 == 0, ME_ERR_BAD_SHAPE,
             "me_op_conv_transpose2x2_pair: %d x %d x %d, %d + %d -> %d", B, H, W, Cin_a, Cin_b, Cout);
    ME_CHECK(act16 == ACT_NONE || act16 == ACT_RELU, ME_ERR_BAD_ARG, "me_op_conv_transpose2x2_pair: act16=%d", act16);
    ME_CHECK(grid_cap >= 0, ME_ERR_BAD_ARG, "me_op_conv_transpose2x2_pair: grid_cap=%d", grid_cap);
    admit_a_wrap("me_op_conv_transpose2x2_pair", Cin_b, a_wrap_b);
}
inline void admit_op_patch_embed(int32_t windows, int32_t P, int32_t C) {
    ME_CHECK(windows > 0 && P > 0 && C > 0 && (int64_t)windows * P < (1 << 30), ME_ERR_BAD_SHAPE,
             "me_op_patch_embed: %d windows of %d patches, dim %d", windows, P, C);
}
// me_op_linear_segments: a weight (and in the residual form a gamma) per segment, the segment starts in order inside the rows
inline void admit_op_linear_segments(int32_t M, int32_t seg1, int32_t seg2, const void* const W16[3], const float* const gamma[3],
                                     bool resid) {
    ME_CHECK(W16[0] && (seg1 == 0 || W16[1]) && (seg2 == 0 || W16[2]), ME_ERR_BAD_ARG,
             "me_op_linear_segments: a row segment without weights");
    admit_row_segments("me_op_linear_segments", seg1, seg2, M);
    if (resid)
        ME_CHECK(gamma && gamma[0] && (seg1 == 0 || gamma[1]) && (seg2 == 0 || gamma[2]), ME_ERR_BAD_ARG,
                 "me_op_linear_segments: the residual form takes gamma for every segment");
}
// me_op_linear_residual_layernorm(_fp8)
inline void admit_op_linear_residual_layernorm(const char* who, int32_t M, int32_t N, int32_t seg1, int32_t seg2, const void* const W16[3],
                                               const float* const bias[3], const float* const gamma[3], const float* const ln_w[3],
                                               const float* const ln_b[3]) {
    admit_row_segments(who, seg1, seg2, M);
    admit_segment_weights(who, seg1, seg2, W16, bias, gamma, ln_w, ln_b);
    ME_CHECK(N == 256 || N == 512 || N == 1024, ME_ERR_BAD_SHAPE, "%s: N = %d not in {256, 512, 1024}", who, N);
}

// ---- the row-segmented attention and LayerNorm entries --------------------------------------------------
// The kernels trust the row map (RowSegs), so a layout that does not fit its buffers is refused here: the windows of each segment,
// `tokens` rows apart from the segment's start, end inside the segment, the last segment's inside rows_total.
inline void admit_op_attention_segments(const uint8_t* out8, int32_t windows, int32_t tokens, int32_t heads, int64_t rows_total,
                                        int64_t seg1, int64_t seg2, int32_t win0, int32_t win1) {
    ME_CHECK(!out8 || heads % 2 == 0, ME_ERR_BAD_ARG, "me_op_attention_segments: fp8 output with %d heads (an odd number)", heads);
    ME_CHECK(windows > 0 && tokens > 0 && heads > 0 && rows_total > 0, ME_ERR_BAD_SHAPE,
             "me_op_attention_segments: windows=%d tokens=%d heads=%d rows=%lld", windows, tokens, heads, (long long)rows_total);
    ME_CHECK(row_segments_ordered(seg1, seg2, rows_total) && win0 >= 0 && win1 >= 0,
             ME_ERR_BAD_ARG, "me_op_attention_segments: segments %lld / %lld of %lld rows, %d / %d windows", (long long)seg1,
             (long long)seg2, (long long)rows_total, win0, win1);
    const int64_t T = tokens, last = (int64_t)windows - win0 - win1;  // windows of the last segment
    bool fits;
    if (seg1 == 0) fits = windows * T <= rows_total;
    else if (seg2 == 0) fits = win0 * T <= seg1 && last == 0 && seg1 + win1 * T <= rows_total;
    else fits = win0 * T <= seg1 && seg1 + win1 * T <= seg2 && last >= 0 && seg2 + last * T <= rows_total;
    ME_CHECK(fits, ME_ERR_BAD_SHAPE, "me_op_attention_segments: %d windows of %d rows (%d / %d in the first segments) do not fit "
             "segments %lld / %lld of %lld rows", windows, tokens, win0, win1, (long long)seg1, (long long)seg2, (long long)rows_total);
}
inline void admit_op_layernorm_segments(const float* const weight[3], const float* const bias[3], int64_t seg1, int64_t seg2,
                                        const uint8_t* y8, int64_t rows, int32_t dim) {
    ME_CHECK(rows > 0, ME_ERR_BAD_SHAPE, "me_op_layernorm_segments: %lld rows", (long long)rows);
    admit_row_segments("me_op_layernorm_segments", seg1, seg2, rows);
    admit_segment_weights("me_op_layernorm_segments", seg1, seg2, weight, bias);
    const bool wide = dim == 256 || dim == 512 || dim == 1024;
    ME_CHECK(wide || (!y8 && (dim == 64 || dim == 128)), ME_ERR_BAD_SHAPE, "me_op_layernorm_segments: dim %d", dim);
}

// ---- the layout / element-wise entries (elementwise.hip): the launch helpers trust the pipeline ----------
inline void admit_grid(const char* who, int32_t grid) {
    ME_CHECK(grid >= 8 && grid <= 64 && grid % 8 == 0, ME_ERR_BAD_SHAPE, "%s: grid %d is not a multiple of 8 in [8, 64]", who, grid);
}
inline void admit_map(const char* who, int32_t batch, int32_t H, int32_t W, int32_t C) {
    ME_CHECK(batch > 0 && batch <= 65535 && H > 0 && W > 0 && C > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)C <= 65535 * 32ll,
             ME_ERR_BAD_SHAPE, "%s: %d x %d x %d x %d", who, batch, H, W, C);
}
inline void admit_op_bilinear(int32_t planes, int32_t in_size, int32_t out_size) {
    ME_CHECK(planes > 0 && in_size > 0 && out_size > 0 && in_size <= 32768 && out_size <= 32768, ME_ERR_BAD_SHAPE,
             "me_op_bilinear: %d planes, %d -> %d", planes, in_size, out_size);
}
inline void admit_op_patchify(int32_t batch, int32_t grid) {
    admit_grid("me_op_patchify", grid);
    ME_CHECK(batch > 0 && batch <= 1024, ME_ERR_BAD_SHAPE, "me_op_patchify: batch %d", batch);
}
inline void admit_op_patchify_windows(int32_t windows, int32_t grid) {
    admit_grid("me_op_patchify_windows", grid);
    ME_CHECK(windows > 0 && windows <= 35 * 1024, ME_ERR_BAD_SHAPE, "me_op_patchify_windows: %d windows", windows);
}
inline void admit_op_cls_rows(int32_t windows, int32_t tpw, int32_t dim) {
    ME_CHECK(windows > 0 && tpw > 0 && dim > 0, ME_ERR_BAD_SHAPE, "me_op_cls_rows: %d windows of %d tokens, dim %d", windows, tpw, dim);
}
inline void admit_op_merge(int32_t batch, int32_t wpi, int32_t win0, int32_t steps, int32_t padding, int32_t grid, int32_t dim) {
    admit_grid("me_op_merge", grid);
    ME_CHECK(batch > 0 && dim > 0 && steps >= 1 && steps <= 5 && padding >= 0 && 2 * padding < grid && (steps > 1 || padding == 0) &&
                 win0 >= 0 && wpi > 0 && win0 + steps * steps <= wpi,
             ME_ERR_BAD_SHAPE, "me_op_merge: batch %d, windows %d + %d x %d of %d, padding %d, dim %d", batch, win0, steps, steps, wpi,
             padding, dim);
}
inline void admit_op_concat_channels(int64_t pixels, int32_t Ca, int32_t Cb) {
    ME_CHECK(pixels > 0 && Ca > 0 && Cb > 0, ME_ERR_BAD_SHAPE, "me_op_concat_channels: %lld pixels of %d + %d channels",
             (long long)pixels, Ca, Cb);
}
inline void admit_op_fov_add(int32_t batch, int32_t grid, int32_t C, int32_t tpw) {
    admit_grid("me_op_fov_add", grid);
    ME_CHECK(batch > 0 && C > 0 && tpw >= grid * grid + 1, ME_ERR_BAD_SHAPE, "me_op_fov_add: batch %d, %d channels, %d tokens per window",
             batch, C, tpw);
}
inline void admit_op_fov_final(int32_t batch, int32_t k, int32_t C) {
    ME_CHECK(batch > 0 && k > 0 && C > 0 && (int64_t)k * k * C < (1ll << 31), ME_ERR_BAD_SHAPE, "me_op_fov_final: batch %d, %d x %d x %d",
             batch, k, k, C);
}

}  // namespace me
