// The launch descriptors of every GEMM, convolution and ConvTranspose form the model runs -- GemmParams, the RowSegs of the
// row-segmented attention and LayerNorm launches -- and their builders: host code, shared by the forward pass (pipeline.hip) and
// the kernel-level entries (api.hip me_op_*), so that the op tests launch what the pipeline launches.  A builder takes operands
// and shapes and fills what the kernels read; which tile runs, split-K, grid_cap and the profiler's flop_rows stay with the
// caller.  Free of HIP and of the context (the one builder that allocates, set_fused_layernorm, has its me_ctx half in model.h), so
// that a host compiler alone can build a descriptor and ask admission.h whether the launchers take it
// (tests/test_admission_cpu.py).  DESIGN.md 4.45.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/matrix_eyes_hip.h"  // ME_ERR_*
#include "error.h"
#include "tile_choice.h"

namespace me {

// D[m][n] = sum_k A(m,k) * W[n][k]  (+ epilogue); AMode and EpiKind: tile_choice.h
enum Act : int32_t { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2 };

struct GemmParams {
    // problem
    int32_t M, N, K;
    // A operand
    const void* A;     // f16/bf16
    int64_t lda;       // elements (A_PLAIN)
    // A_CONV geometry: input map [B][Hp][Wp][Cin] with Hp = Hin + 2, Wp = Win + 2 (zero border)
    int32_t in_Hp, in_Wp, Cin;
    int32_t out_H, out_W;     // output pixels per image: M = B * out_H * out_W
    int32_t KH, KW, stride;   // 1x1 or 3x3 (pad (KH-1)/2); stride 1 or 2
    // W operand
    const void* W;     // [N][K]
    // epilogue
    const float* bias;     // [N] or [Cout] (EPI_CONVT) or null
    const float* gamma;    // EPI_RESID_SCALE
    const float* res32;    // optional f32 residual, same row mapping as out32
    const float* res32b;   // optional second f32 residual
    const float* pos;      // EPI_PATCH_EMBED: pos_embed [P+1][N]
    float* out32;          // optional f32 output
    void* out16;           // optional f16/bf16 output
    int64_t ldc;           // row stride (elements) of out32/out16/res32 for row-major outputs
    int64_t ldc16;         // row / pixel stride of out16 when it differs from ldc (0: same)
    // Split 16-bit output (pipeline.hip "split operands"): besides hi = T(v) at its place, lo = T(v - hi) is
    // stored lo_off16 elements further on, so that a consumer whose K axis reads [hi | lo] against
    // duplicated weights sees v to ~2^-22 instead of 2^-11.  0: plain 16-bit output.
    int32_t lo_off16;
    int32_t hi2_off16;     // with lo_off16: a second copy of hi this many elements on ([hi | lo | hi] operands)
    int32_t act;           // activation applied to the f16 output (and f32 for EPI_STORE)
    int32_t act16_only;    // 1: activation only on the out16 copy (out32 stays raw)
    int32_t out16_border;  // EPI_STORE/EPI_CONVT: out16 is zero-bordered [B][out_H+2][out_W+2][C]
    int32_t tokens_per_window;  // EPI_PATCH_EMBED: P
    int32_t Cout;          // EPI_CONVT: N = 4*Cout
    // EPI_HEAD_FINAL
    // f32 [9][ld]: the share of each 3x3 tap in `bias`, taken out again where the tap falls into the zero padding of a layer that
    // was composed into this convolution at load time (weights.hip compose_head: EPI_HEAD_COMPOSED, ld = 32; compose_features: the
    // halo tile's EPI_STORE with a bordered 16-bit output, ld = N)
    const float* tap_bias;
    const float* w2;       // [N]
    const float* b2;       // device scalar
    const float* f_norm;   // device [B] (one per image) or null (= 1): out32[m] = clamp(v / f_norm[b])
    float clamp_lo, clamp_hi;  // mod.rs:362 clamp(1e-4, 1e4); +-inf for the canonical head output
    int32_t pixels_per_image;
    // diagnostic builds only (tools/gemm_stamps.py): per-workgroup s_memrealtime stamps, or null
    unsigned long long* stamps;
    // Row segments with their own weights (the three ViTs of the encoder in one launch, pipeline.hip):
    // rows [0, seg1) use W / bias / gamma, [seg1, seg2) the *_s1 set, [seg2, M) the *_s2 set.  seg1 == 0:
    // one segment.  seg2 == 0: two.  Both must be multiples of the tile height (checked at launch).
    int32_t seg1, seg2;
    const void *W_s1, *W_s2;
    const float *bias_s1, *bias_s2, *gamma_s1, *gamma_s2;
    // MX fp8 operands (gemm_fp8.hip): e8m0 block scales of A and W in the per-wave layouts of mx_fp8.h, a_mt =
    // 128-row tiles of the A scale array; fp8 output (the next GEMM's A operand) with its scale array
    const uint8_t *a_scale, *w_scale, *w_scale_s1, *w_scale_s2;
    int32_t a_mt;
    uint8_t *out8, *out8_scale;
    int32_t out8_mt;
    // Algorithmic work of the launch for the profiler (bench.py's roofline): rows that belong to real tokens /
    // pixels (0: M; the merged ViT row space pads each segment to 256 rows) and the K of the layer itself (0: K; a
    // split [hi | lo] operand doubles or triples the K the kernel walks without adding algorithmic FLOPs)
    int32_t flop_rows, flop_k;
    // Context status word (me_status_flags): bit 0 is set when an f16 operand store met a magnitude beyond 65504
    // (gemm_launch fills it in from the calling context)
    unsigned* status;
    // tile rows of an XCD's patch in the tile walk (gemm_core.h tile_origin); 0: 8
    int32_t patch_rows;
    // EPI_STORE, 16-bit output without activation (the qkv linear, vit.rs:58-62): columns n < qcols leave multiplied
    // by qscale -- Q of the attention kernel arrives scaled by 1/sqrt(head_dim) * log2(e) with ONE rounding, the
    // product (acc + bias) * qscale rounded to 16 bits, instead of being scaled and rounded again where it is
    // consumed (attention.hip attention2_kernel).  qcols == 0: off.  A multiple of 64 (whole heads).
    int32_t qcols;
    float qscale;
    // LayerNorm of the updated token rows inside EPI_RESID_SCALE (gemm_core.h resid_ln_epilogue; the 352-row tile, N in
    // {256, 512, 1024}): besides x += gamma * (A W^T + b) the launch writes ln_out16[m][:] = LayerNorm(x[m][:]) * w + b
    // with the weights of the row's segment -- the next linear's operand (vit.rs:165-169: norm1 / norm2 of Block::forward).
    // The N / 256 column tiles of a row tile exchange their partial (mean, M2) through ln_stats ([row tile][column tile]
    // [352] 8-byte granules) and count their arrivals in ln_count (one word per row tile, 64 bytes apart; the count only
    // ever grows by N / 256 per launch, so it needs no reset between launches or graph replays).  ln_out16 == null: off.
    void* ln_out16;
    const float *ln_w, *ln_b, *ln_w_s1, *ln_b_s1, *ln_w_s2, *ln_b_s2;
    float ln_eps;
    unsigned long long* ln_stats;
    unsigned* ln_count;
    // polls a workgroup spends waiting for its row tile's other column tiles before it raises ME_STATUS_SYNC_TIMEOUT
    // (0: 2^20, about 2 s; gemm_launch fills it in from ME_LN_SPIN_LIMIT, a test knob)
    int32_t ln_spin_limit;
    // compute units the launch stream may use when that is fewer than the device has (a stream created with a CU mask;
    // gemm_launch fills it in, gemm.hip stream_cu_count): persistent grids are sized from it.  0: all of them
    int32_t cu_granted;
    // query form (gemm.hip gemm_lnf_resident): the launcher writes the number of workgroups it would keep resident
    // here and returns without launching.  Host pointer; null for a launch
    int32_t* resident_out;
    // development A/B (ME_GELU_BATCH=0): fc1's GELU four values at a time instead of a pass's sixteen at once
    int32_t gelu_per_granule;
    // persistent kernels: at most this many workgroups (a multiple of 8), so that a launch on another stream finds
    // free CUs beside this one; 0: as many as are resident
    int32_t grid_cap;
    // Deterministic split-K (gemm_core.h gemm_kernel<..., SPLITK>; the 128x128 tile, EPI_STORE): split_k > 1 work items per tile,
    // each over a K range; every one writes its f32 partial (accumulator layout) to splitk_ws[(tile * split_k + s)][BM * BN] and
    // counts its arrival in splitk_cnt[tile] (zero before the launch; the last arriver resets it); the LAST arriver sums the
    // partials in split order -- its own included, so the result does not depend on who is last -- and runs the epilogue.
    int32_t split_k;
    float* splitk_ws;
    unsigned* splitk_cnt;
    // Tile queue of the launch stream (gemm_launch fills it in), or null for the static tile order.
    // Word 32 x: next-tile ticket of XCD x (x < 8), word 256: exited workgroups -- one 128-byte line each
    // (on one line the 512 prologue draws of a launch serialise in a single L2 channel).
    unsigned* queue;
    // (the members below stand behind everything older kernels read: their kernel-argument offsets stay what they were)
    // A_PLAIN rows whose last part repeats their first ([hi | lo | hi] operands, gemm_params.h set_a_parts): K slabs
    // kt >= a_wrap are read from slab kt - a_wrap of the row, which is then stored a_wrap * 64 elements wide.  0: no wrap.
    // EPI_CONVT only (the one consumer of such operands).
    int32_t a_wrap;
    // Chained second operand set (gemm_core.h gemm_pp_kernel<..., CHAIN>; the 256x256 two-group tile, EPI_CONVT, gemm_params.h
    // chain_convt): a tile runs the K loop of (A, W, K), stores the 16-bit output act(acc + bias) from the accumulators, runs
    // the K loop of (A2, W2, K2) on the SAME accumulators and stores out32 = acc + bias2 -- two ConvTransposes over one input
    // grid summed in one accumulator.  A2 == null: an ordinary launch.
    const void *A2, *W2;
    int64_t lda2;
    int32_t K2, a_wrap2, flop_k2;
    const float* bias2;
};
constexpr int kGemmQueueWords = 9 * 32;

// Row segments of the encoder's merged ViT launches (pipeline.hip): segment 0 = rows [0, seg1), 1 =
// [seg1, seg2), 2 = [seg2, ...).  Windows are contiguous (stride `tokens` rows) inside a segment; win0 /
// win1 are the numbers of windows of segments 0 and 1.  seg1 == 0: no segmentation.
struct RowSegs {
    int64_t seg1 = 0, seg2 = 0;
    int32_t win0 = 0, win1 = 0;
    const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;  // LayerNorm weights of 1 and 2
};
// 1/sqrt(head_dim) (vit.rs:47) times log2(e): the factor a pre-scaled Q carries (GemmParams::qscale of the qkv launch)
constexpr float kAttnQScale = 0.125f * 1.44269504088896340736f;

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
// allocated, never reset: it advances by N / 256 per launch, so launches of different N must not share one).  The caller
// brings both, of the sizes ln_scratch_bytes states (model.h set_fused_layernorm(me_ctx*, ...) takes them from the context).
struct LnScratchBytes {
    uint64_t stats, count;
};
inline LnScratchBytes ln_scratch_bytes(const GemmParams& p) {
    const uint64_t row_tiles = (uint64_t)seg_row_tiles<352>(p.M, p.seg1, p.seg2);
    return {row_tiles * (uint64_t)(p.N / 256) * 352 * 8, row_tiles * 64};
}
inline void set_fused_layernorm(GemmParams& p, const LnSet& ln, float eps, void* xn16, uint8_t* xn8, uint8_t* xn_scale,
                                unsigned long long* ln_stats, unsigned* ln_count) {
    p.ln_out16 = xn8 ? (void*)xn8 : xn16, p.ln_eps = eps;  // (ln_out16 != null is the kernels' switch, fp8 or not)
    if (xn8) set_out8(p, xn8, xn_scale);
    p.ln_w = ln.w0, p.ln_b = ln.b0, p.ln_w_s1 = ln.w1, p.ln_b_s1 = ln.b1, p.ln_w_s2 = ln.w2, p.ln_b_s2 = ln.b2;
    p.ln_stats = ln_stats, p.ln_count = ln_count;
}

}  // namespace me
