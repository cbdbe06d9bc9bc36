// The Depth Pro forward pass as a sequence of HIP kernel launches on one stream.
// Stage structure follows reference src/depth_pro/mod.rs:251-363; each function cites the
// module forward() it replaces.  Activations live in HBM as:
//   - ViT: f32 residual stream [windows*tokens][C] + 16-bit GEMM operands
//   - conv stages: NHWC; 16-bit operands of 3x3 convs carry a 1-pixel zero border
//     ([B][H+2][W+2][C]) so the implicit-GEMM loader needs no bounds checks, residual paths
//     stay f32 ([B*H*W][C]).
#include <algorithm>
#include <memory>

#include "model.h"

namespace me {

void report(me_ctx* ctx, float pos, const char* msg) {
    if (ctx->progress)
        ctx->progress(ctx->progress_user, ctx->prog_lo + pos * (ctx->prog_hi - ctx->prog_lo), msg);
}

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // plain malloc'd host memory is "invalid value": not an error
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

void* site_buf(me_ctx* ctx, const std::string& name, size_t bytes) {
    DevBuf& b = ctx->bufs[name];
    if (b.p && b.bytes >= bytes) return b.p;
    if (ctx->capturing) throw CaptureAbort();  // an allocation would synchronise: the caller runs eagerly instead
    if (b.p) {
        ME_HIP(hipStreamSynchronize(ctx->stream));
        ctx->drop_graph();  // a captured step may hold the old address (dropped once its replays have drained)
        ME_HIP(hipFree(b.p));
        b.p = nullptr, b.bytes = 0;
    }
    ME_HIP(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    ME_HIP(hipMemsetAsync(b.p, 0, bytes, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    return b.p;
}

const void* to_device(me_ctx* ctx, const void* p, size_t bytes, const std::string& name) {
    if (is_device_ptr(p)) return p;
    void* d = site_buf(ctx, name, bytes);
    ME_HIP(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    return d;
}

void from_device(me_ctx* ctx, void* dst, const void* src_dev, size_t bytes) {
    if (is_device_ptr(dst)) {
        if (dst != src_dev)
            ME_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        ME_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        ME_HIP(hipStreamSynchronize(ctx->stream));
    }
}

namespace {

// ---- thin launch helpers: the descriptors come from gemm_params.h, the launch decisions from tile_choice.h ----
// Deterministic split-K for the small deep launches of the tail (tile_choice.h split_k_factor): the workspace of the launch.
// Returns the tile configuration to force (CFG_128) or -1.
int maybe_split_k(me_ctx* ctx, GemmParams& p, int64_t rows_per_image, hipStream_t s) {
    const int S = split_k_factor(rows_per_image, p.M, p.N, p.K, tile_knobs());
    if (S == 1) return -1;
    const int64_t tiles = cdiv((int64_t)p.M, 128) * cdiv((int64_t)p.N, 128);
    // one workspace per stream (launches of one stream follow one another; a second stream must not share it)
    const std::string tag = "splitk." + std::to_string((uintptr_t)s);
    p.split_k = S;
    p.splitk_ws = (float*)site_buf(ctx, tag + ".ws", (size_t)tiles * S * 128 * 128 * 4);   // grows to the largest launch
    p.splitk_cnt = (unsigned*)site_buf(ctx, tag + ".cnt", 4096 * 4);   // zero when allocated; the last arriver of a tile resets its word
    return CFG_128;
}

// out = act(A[M][K] . W[N][K]^T + bias) as 16-bit and/or f32 rows of N (split operands, model.h SplitStage: a_split: A holds
// [hi | lo] rows of 2K and W is stored [W | W]; out_split: the 16-bit output is written as [hi | lo] rows of 2N)
// rows_per_image > 0: the launch may take the split-K form (maybe_split_k)
void linear(me_ctx* ctx, const void* A, int64_t M, int K, const void* W, int N, const float* bias,
            void* out16, float* out32, int act, hipStream_t s, bool a_split = false,
            bool out_split = false, int qcols = 0, int64_t rows_per_image = 0) {
    GemmParams p = linear_params(M, N, K, A, W, bias, out16, out32, act);
    set_a_parts(p, a_split ? 2 : 1);
    set_out16_parts(p, N, out_split ? 2 : 1);
    set_scaled_cols(p, qcols, kAttnQScale);  // the qkv linear: Q leaves scaled for the attention kernel
    p.grid_cap = ctx->grid_cap;
    gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, s, maybe_split_k(ctx, p, rows_per_image, s));
}

// Conv2d k x k (k = 1 or 3, pad (k-1)/2, stride 1 or 2) on a zero-bordered NHWC operand
void conv(me_ctx* ctx, const void* in16b, int B, int Hin, int Win, int Cin, const void* W, int Cout,
          int k, int stride, const float* bias, const ConvOut& o, hipStream_t s, bool a_split = false) {
    GemmParams p = conv_params(in16b, B, Hin, Win, Cin, W, Cout, k, stride, bias, o, a_split);
    p.grid_cap = ctx->grid_cap;
    gemm_launch(p, A_CONV, EPI_STORE, ctx->dtype, s, o.tap_bias ? -1 : maybe_split_k(ctx, p, (int64_t)p.out_H * p.out_W, s));
}

// ConvTranspose2d(2,2,stride 2) of an unbordered NHWC operand [B*H*W][Cin] -> [B][2H][2W][Cout]: the arguments of convt_params
void convt(me_ctx* ctx, const void* in16, int B, int H, int W_, int Cin, const void* W, int Cout,
           const float* bias, float* out32, void* out16, bool border16, int64_t pixel_stride,
           int act16, hipStream_t s, bool a_split = false, bool out_split = false, int64_t lo_off = 0,
           int k_copies = 0, bool wrap_third = false) {
    GemmParams p = convt_params(in16, B, H, W_, Cin, W, Cout, bias, out32, out16, border16, pixel_stride, act16, a_split,
                                out_split, lo_off, k_copies, wrap_third);
    p.grid_cap = ctx->grid_cap;
    gemm_launch(p, A_PLAIN, EPI_CONVT, ctx->dtype, s);
}

size_t bordered_bytes(int B, int H, int W, int C) { return (size_t)B * (H + 2) * (W + 2) * C * 2; }

// encoder.rs:210-216 forward_seq over an upsample block: 1x1 conv (no bias) then ConvT x n.
// The last ConvT writes the caller's outputs.  With SPLIT_UPSAMPLE the input and every intermediate are
// [hi | lo] operands; last_split / last_lo_off say whether (and where) the last 16-bit output is split too.
// skip_last (me_ctx::enc0_sum): the chain stops before its last ConvT and leaves that launch's operand in the context
void run_upsample(me_ctx* ctx, const std::string& tag, const void* in16, int B, int H,
                  const UpsampleW& u, float* last32, void* last16, bool last_border,
                  int64_t last_pixel_stride, int last_act16, hipStream_t s, bool last_split = false,
                  int64_t last_lo_off = 0, bool skip_last = false) {
    const int C = ctx->C();
    const bool sp = ctx->split(SPLIT_UPSAMPLE);
    const int64_t M = (int64_t)B * H * H;
    const size_t wide = sp ? 2 : 1;
    void* a = site_buf(ctx, tag + ".proj", (size_t)M * u.dim_int * 2 * wide);
    linear(ctx, in16, M, C, u.conv, u.dim_int, nullptr, a, nullptr, ACT_NONE, s, sp, sp, 0, (int64_t)H * H);
    const void* cur = a;
    int h = H;
    const int n = (int)u.convt.size();
    for (int i = 0; i < n; ++i) {
        const bool last = i == n - 1;
        if (last && skip_last) {
            ctx->enc0_last_in = cur, ctx->enc0_last_side = h;
        } else if (last) {
            convt(ctx, cur, B, h, h, u.cin[i], u.convt[i], u.cout[i], nullptr, last32, last16,
                  last_border, last_pixel_stride, last_act16, s, sp, last_split, last_lo_off);
        } else {
            void* t = site_buf(ctx, tag + ".up" + std::to_string(i),
                               (size_t)B * 4 * h * h * u.cout[i] * 2 * wide);
            convt(ctx, cur, B, h, h, u.cin[i], u.convt[i], u.cout[i], nullptr, nullptr, t, false, 0,
                  ACT_NONE, s, sp, sp);
            cur = t;
        }
        h *= 2;
    }
}

struct TapCtx {
    me_ctx* ctx;
    int B;
    void *lat0, *lat1;
    hipStream_t s;
};

void tap_fn(void* user, int index, const float* tokens) {
    TapCtx* t = (TapCtx*)user;
    me_ctx* ctx = t->ctx;
    // encoder.rs:266-280: reshape_feature + merge of the first 25 windows, padding 3 (= g/8)
    // vit.rs:311-316 pushes a tapped block's output when the loop REACHES it (`blocks_to_take.contains(&i)`), so output[0] --
    // latent0 -- is the earlier of the two blocks whatever the order they are listed in
    const int t0 = ctx->cfg.tap_blocks[0], t1 = ctx->cfg.tap_blocks[1];
    void* dst = index == (t0 < t1 ? t0 : t1) ? t->lat0 : (index == (t0 < t1 ? t1 : t0) ? t->lat1 : nullptr);
    if (dst)
        merge_launch(tokens, nullptr, dst, t->B, 35, 0, 5, ctx->g() / 8, ctx->g(), ctx->C(),
                     ctx->dtype, t->s, ctx->split(SPLIT_UPSAMPLE) ? 1 : 0);
}

}  // namespace

// vit.rs:287-346: prepare_tokens_with_mask, 24 x Block::forward, final LayerNorm -- as an object, so
// that the encoder can issue the three ViTs block by block in turn (see stage_encoder).
namespace {
struct VitRun {
    me_ctx* ctx;
    const VitW& v;
    int W;
    VitTaps taps;
    hipStream_t s;
    int64_t rows;
    float* tok;
    void *xn, *qkv, *att, *hid;

    // vit.rs:287-295: patch embed + cls + pos
    VitRun(me_ctx* ctx_, int which, const void* patches16, int W_, const VitTaps& taps_, const std::string& tag,
           hipStream_t s_)
        : ctx(ctx_), v(ctx_->w.vit[which]), W(W_), taps(taps_), s(s_) {
        const int C = ctx->C(), T = ctx->T(), P = ctx->P();
        rows = (int64_t)W * T;
        tok = (float*)site_buf(ctx, tag + ".tokens", (size_t)rows * C * 4);
        xn = site_buf(ctx, tag + ".xn", (size_t)rows * C * 2);
        qkv = site_buf(ctx, tag + ".qkv", (size_t)rows * 3 * C * 2);
        att = site_buf(ctx, tag + ".att", (size_t)rows * C * 2);
        hid = site_buf(ctx, tag + ".hid", (size_t)rows * 4 * C * 2);
        cls_rows_launch(tok, v.cls, v.pos, W, T, C, s);
        gemm_launch(patch_embed_params(W, P, C, patches16, v.patch_w, v.patch_b, v.pos, tok), A_PLAIN, EPI_PATCH_EMBED, ctx->dtype, s);
    }

    // vit.rs:163-170 Block::forward
    void block(int i) {
        const VitBlockW& b = v.blocks[i];
        const int C = ctx->C(), T = ctx->T(), heads = ctx->cfg.num_heads;
        layernorm_launch(tok, b.ln1_w, b.ln1_b, xn, nullptr, rows, C, ctx->cfg.ln_eps, ctx->dtype, s);
        linear(ctx, xn, rows, C, b.qkv_w, 3 * C, b.qkv_b, qkv, nullptr, ACT_NONE, s, false, false, C);
        attention_launch(qkv, att, W, T, heads, ctx->dtype, s, nullptr, nullptr, nullptr, 0, true);
        gemm_launch(resid_params(rows, C, C, att, b.proj_w, b.proj_b, b.ls1, tok), A_PLAIN, EPI_RESID_SCALE, ctx->dtype, s);
        layernorm_launch(tok, b.ln2_w, b.ln2_b, xn, nullptr, rows, C, ctx->cfg.ln_eps, ctx->dtype, s);
        linear(ctx, xn, rows, C, b.fc1_w, 4 * C, b.fc1_b, hid, nullptr, ACT_GELU, s);
        gemm_launch(resid_params(rows, C, 4 * C, hid, b.fc2_w, b.fc2_b, b.ls2, tok), A_PLAIN, EPI_RESID_SCALE, ctx->dtype, s);
        if (taps.fn) taps.fn(taps.user, i, tok);
    }

    // vit.rs:343 final norm
    void finish(void* final16, float* final32) {
        layernorm_launch(tok, v.norm_w, v.norm_b, final16, final32, rows, ctx->C(), ctx->cfg.ln_eps, ctx->dtype, s);
    }
};

// The encoder's three ViTs (patch encoder on 35 B windows, image encoder and FOV encoder on B windows each,
// different weights, same architecture) as ONE row space: segment 0 = the patch encoder's rows, 1 = the
// image encoder's, 2 = the FOV encoder's, each padded to a multiple of 256 rows so that no GEMM tile
// straddles two weight sets.  Every kernel of a block then runs ONCE over all rows, with the weights chosen
// per row tile (GEMMs, GemmParams::seg1/seg2), per row (LayerNorm) or not at all (attention: a window ->
// row map).  qkv: 948 + 72 tiles still fit the four rounds the patch encoder needs alone; fc1 goes from
// 4.94 to 5.31 rounds, which costs what the separate small launches did; proj / fc2 move to the 256x256
// tile (see resid_all).  This replaces two side streams of ~170 small launches each, which took CUs from
// the launch stream's persistent kernels at every kernel boundary (fc2 0.195 -> 0.34 ms on most layers):
// 26.5 -> 25.5 ms per step, 580 -> 390 launches.
struct MergedVit {
    me_ctx* ctx;
    const VitW &v0, &v1, &v2;  // patch encoder, image encoder, FOV encoder
    // Physical order of the row space: the SMALL segments first -- [image encoder | FOV encoder | patch encoder]
    // (without the FOV head: [image encoder | patch encoder]).  Every boundary is then a multiple of the small
    // segments' padded length (768 rows at one image: a multiple of 256 AND of 192, so the 192-row residual tile
    // can be used), and the one ragged end is the end of the row space, which every kernel clamps anyway.
    const VitW &p0, &p1, &p2;  // the ViT of physical segment 0, 1, 2 (p2 unused without the FOV head)
    int W0, W1;        // windows of the patch encoder and of each small ViT
    bool fov;
    VitTaps taps;
    hipStream_t s;
    int64_t R0, seg1, seg2, Rtot;  // rows of the patch encoder; starts of physical segments 1 and 2 (seg2 == 0: two)
    int64_t row_main, row_img, row_fov;  // first row of each ViT
    float* tok;
    char *xn, *qkv, *att, *hid, *fin16;
    bool xn_is_norm1 = false;  // xn already holds norm1 of the block about to run (written by the block before)
    bool xn_is_norm1_fp8 = false;  // fp8 contexts: xn / xn_s hold norm1 of the block about to run as MX fp8 (the fp8 fc2's epilogue)
    bool xn_is_norm2_fp8 = false;  // fp8 contexts: xn / xn_s hold norm2 as MX fp8 (written by the projection's epilogue)
    float* fin32 = nullptr;
    // ME_DTYPE_FP8: xn and hid hold e4m3 bytes, with their block scales (activation layout, Rtot / 128 tiles)
    uint8_t *xn_s = nullptr, *hid_s = nullptr, *att8 = nullptr, *att_s = nullptr;
    RowSegs segs;

    static int64_t pad256(int64_t r) { return (r + 255) / 256 * 256; }
    // rows that hold tokens (the profiler's algorithmic FLOPs; the padding rows of each segment are not work)
    int64_t real_rows() const { return (int64_t)(W0 + W1 * (fov ? 2 : 1)) * ctx->T(); }

    MergedVit(me_ctx* ctx_, int B, bool fov_, const void* patches_main, const void* patches_img,
              const void* patches_fov, const VitTaps& taps_, hipStream_t s_)
        : ctx(ctx_), v0(ctx_->w.vit[ME_VIT_PATCH_ENCODER]), v1(ctx_->w.vit[ME_VIT_IMAGE_ENCODER]),
          v2(ctx_->w.vit[ME_VIT_FOV_ENCODER]), p0(v1), p1(fov_ ? v2 : v0), p2(v0), W0(35 * B), W1(B), fov(fov_),
          taps(taps_), s(s_) {
        const int C = ctx->C(), T = ctx->T(), P = ctx->P();
        R0 = (int64_t)W0 * T;
        const int64_t side = pad256((int64_t)W1 * T);
        seg1 = side;
        seg2 = fov ? 2 * side : 0;
        row_img = 0, row_fov = fov ? side : -1, row_main = fov ? 2 * side : side;
        Rtot = row_main + pad256(R0);
        tok = (float*)site_buf(ctx, "vitm.tokens", (size_t)Rtot * C * 4);
        xn = (char*)site_buf(ctx, "vitm.xn", (size_t)Rtot * C * 2);
        qkv = (char*)site_buf(ctx, "vitm.qkv", (size_t)Rtot * 3 * C * 2);
        att = (char*)site_buf(ctx, "vitm.att", (size_t)Rtot * C * 2);
        hid = (char*)site_buf(ctx, "vitm.hid", (size_t)Rtot * 4 * C * 2);
        if (ctx->fp8) {
            xn_s = (uint8_t*)site_buf(ctx, "vitm.xn.scale", (size_t)Rtot * C / 32);
            hid_s = (uint8_t*)site_buf(ctx, "vitm.hid.scale", (size_t)Rtot * 4 * C / 32);
            att8 = (uint8_t*)site_buf(ctx, "vitm.att8", (size_t)Rtot * C);
            att_s = (uint8_t*)site_buf(ctx, "vitm.att.scale", (size_t)Rtot * C / 32);
        }
        fin16 = (char*)site_buf(ctx, "vitm.final16", (size_t)Rtot * C * 2);
        // attention: windows of physical segments 0 and 1, the rest belong to the last segment
        segs.seg1 = seg1, segs.seg2 = seg2, segs.win0 = W1, segs.win1 = fov ? W1 : W0;
        // vit.rs:287-295 per ViT: patch embed + cls + pos into its segment
        embed(v0, patches_main, W0, row_main);
        embed(v1, patches_img, W1, row_img);
        if (fov) embed(v2, patches_fov, W1, row_fov);
        // The padding rows of each segment take part in every row-wise kernel of a block (x += gamma * (...),
        // 48 times per call) and the buffer outlives the call: zeroed here, they hold the same finite values on
        // every call instead of growing without bound or keeping another batch size's rows.
        zero_rows(row_img + (int64_t)W1 * T, row_img + side);
        if (fov) zero_rows(row_fov + (int64_t)W1 * T, row_fov + side);
        zero_rows(row_main + R0, Rtot);
        (void)P;
    }

    void zero_rows(int64_t r0, int64_t r1) {
        if (r1 > r0) ME_HIP(hipMemsetAsync(tok + r0 * ctx->C(), 0, (size_t)(r1 - r0) * ctx->C() * 4, s));
    }

    void embed(const VitW& v, const void* patches16, int W, int64_t row) {
        const int C = ctx->C(), T = ctx->T(), P = ctx->P();
        cls_rows_launch(tok + row * C, v.cls, v.pos, W, T, C, s);
        gemm_launch(patch_embed_params(W, P, C, patches16, v.patch_w, v.patch_b, v.pos, tok + row * C), A_PLAIN, EPI_PATCH_EMBED,
                    ctx->dtype, s);
    }

    void set_ln(const float* w1, const float* b1, const float* w2, const float* b2) {
        segs.w1 = w1, segs.b1 = b1, segs.w2 = w2, segs.b2 = b2;
    }

    // Whole rounds + a short tail (tile_choice.h short_tail_rows1): the first rows1 rows on the 256x256 tile, the rest -- all of the last
    // row segment -- as a second launch of 96-row tiles with that segment's weights
    void launch_with_short_tail(const GemmParams& p, EpiKind epi, int64_t rows1) {
        const int64_t rows2 = p.M - rows1;
        GemmParams a = p, b = p;
        a.M = (int)rows1;
        a.flop_rows = (int)std::min<int64_t>(real_rows(), rows1);
        b.M = (int)rows2;
        b.flop_rows = (int)std::max<int64_t>(0, real_rows() - rows1);
        b.A = (const char*)p.A + rows1 * p.lda * 2;
        if (p.out16) b.out16 = (char*)p.out16 + rows1 * p.ldc * 2;
        if (p.out32) b.out32 = p.out32 + rows1 * p.ldc;
        if (p.res32) b.res32 = p.res32 + rows1 * p.ldc;
        b.seg1 = b.seg2 = 0;  // one weight set: the last segment's
        if (p.seg2) b.W = p.W_s2, b.bias = p.bias_s2, b.gamma = p.gamma_s2;
        else if (p.seg1) b.W = p.W_s1, b.bias = p.bias_s1, b.gamma = p.gamma_s1;
        gemm_launch(a, A_PLAIN, epi, ctx->dtype, s, CFG_PP256);
        gemm_launch(b, A_PLAIN, epi, ctx->dtype, s, CFG_PP96);
    }

    // the weights of block i's three physical segments: one linear's members of VitBlockW (gamma: the residual forms)
    template <class Wt>
    SegWeights weights(int i, Wt VitBlockW::*w, const float* VitBlockW::*bias, const float* VitBlockW::*gamma = nullptr,
                       const uint8_t* VitBlockW::*w_scale = nullptr) const {
        const VitBlockW* b[3] = {&p0.blocks[i], &p1.blocks[i], &p2.blocks[i]};
        SegWeights sw;
        for (int k = 0; k < 3; ++k)
            sw.W[k] = b[k]->*w, sw.bias[k] = b[k]->*bias, sw.gamma[k] = gamma ? b[k]->*gamma : nullptr,
            sw.w_scale[k] = w_scale ? b[k]->*w_scale : nullptr;
        return sw;
    }

    // one GEMM over all segments (three weight sets): 16-bit output (qkv, fc1) ...
    void gemm_all(const void* A, int K, const SegWeights& w, int N, void* out16, int act, int qcols = 0) {
        GemmParams p = linear_params(Rtot, N, K, A, nullptr, nullptr, out16, nullptr, act);
        set_segments(p, seg1, seg2, w);
        set_scaled_cols(p, qcols, kAttnQScale);  // qkv: Q leaves scaled for the attention kernel
        p.flop_rows = (int)real_rows();
        const VitLinearPlan plan = vit_linear_plan(p.M, N, K, seg1, seg2, ctx->C(), false, false, false, tile_knobs());
        if (plan.kind == VIT_ROUNDS_TAIL) launch_with_short_tail(p, EPI_STORE, plan.rows1);
        else gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, s, plan.cfg);
    }
    // ... or the residual update x += gamma * (A W^T + b) (proj, fc2).  On the two-group 256x256 tile: the
    // patch encoder's rows alone take 160x128 (two exact rounds), but with the small segments' 24 tiles more
    // the 340 tiles of 256x256 (two rounds) win: 25.5 vs 26.0 ms per step against separate launches.
    // The residual update and the LayerNorm behind it in one launch (gemm_core.h resid_ln_epilogue): 16-bit contexts, the
    // 352-row tile, C in {256, 512, 1024}.  When it applies it applies at EVERY batch size (the tall tile is then taken
    // whatever tall_tile_wins says), so that a row's statistics are summed in the same order whatever batch the row is
    // part of: a batch stays a loop of batch-one calls bit for bit.  ME_LN_FUSE=0: the stand-alone LayerNorm launches.
    // fp8_gemm: the launch that would carry it is gemm8's (gemm_fp8.hip's tall kernel), not resid_all's 16-bit one.
    bool ln_fusable(bool fp8_gemm) const {
        static const bool enabled = env_on("ME_LN_FUSE");
        const int C = ctx->C();
        if (!(enabled && tile_knobs().tall && !tile_knobs().pp192 && (C == 256 || C == 512 || C == 1024))) return false;
        // the context has seen the exchange time out (api.hip run_with_ln_fallback): stand-alone LayerNorm from then on
        if (ctx->ln_fuse_off) return false;
        // one row tile per XCD with all its column tiles must be resident at once on the CUs the stream may use
        // (a smaller part, a partition mode, a stream with a CU mask): otherwise the stand-alone LayerNorm
        return (fp8_gemm ? gemm_fp8_lnf_resident(s) : gemm_lnf_resident(ctx->dtype, s)) >= 8 * (C / 256);
    }
    // returns true when xn holds LayerNorm(ln) of the updated rows
    bool resid_all(const char* A, int K, const SegWeights& w, const LnSet* ln = nullptr,
                   bool ln_fp8 = false /* xn / xn_s as the MX fp8 operand of the next GEMM */) {
        const int C = ctx->C();
        GemmParams p = resid_params(Rtot, C, K, A, nullptr, nullptr, nullptr, tok);
        set_segments(p, seg1, seg2, w);
        p.flop_rows = (int)real_rows();
        const bool ln_wanted = ln && (ln_fp8 || !ctx->fp8);
        const VitLinearPlan plan = vit_linear_plan(p.M, C, K, seg1, seg2, C, true, ln_wanted, ln_wanted && ln_fusable(false), tile_knobs());
        if (plan.kind == VIT_FUSED_LN_352)
            set_fused_layernorm(ctx, p, "vitm.ln.stats", "vitm.ln.count", *ln, ctx->cfg.ln_eps, xn, ln_fp8 ? (uint8_t*)xn : nullptr, xn_s);
        if (plan.kind == VIT_ROUNDS_TAIL) launch_with_short_tail(p, EPI_RESID_SCALE, plan.rows1);
        else gemm_launch(p, A_PLAIN, EPI_RESID_SCALE, ctx->dtype, s, plan.cfg);
        return plan.kind == VIT_FUSED_LN_352;
    }

    // the MX fp8 form of gemm_all / resid_all (gemm_fp8.hip): A = xn or hid as e4m3 + block scales
    // ln (fc2 / proj only): also write LayerNorm(ln) of the updated rows into xn / xn_s as MX fp8 -- the tall tile's residual
    // epilogue; returns true when it did
    bool gemm8(const void* A8, const uint8_t* As, int K, int N, const SegWeights& w, int which /*0 qkv, 1 fc1, 2 fc2, 3 proj*/,
               bool hid16_out = false, const LnSet* ln = nullptr) {
        GemmParams p = which >= 2 ? resid_params(Rtot, N, K, A8, nullptr, nullptr, nullptr, tok)
                                  : linear_params(Rtot, N, K, A8, nullptr, nullptr, nullptr, nullptr);
        set_segments(p, seg1, seg2, w);
        set_fp8_operands(p, As, w.w_scale[0]);
        p.flop_rows = (int)real_rows();
        if (which == 0) {
            p.out16 = qkv;
            set_scaled_cols(p, ctx->C(), kAttnQScale);
            gemm_fp8_launch(p, EPI_STORE, s);
        } else if (which == 1) {
            p.act = ACT_GELU;
            if (hid16_out) p.out16 = hid;  // fc2 stays 16-bit: the hidden layer leaves as f16
            else set_out8(p, (uint8_t*)hid, hid_s);
            gemm_fp8_launch(p, EPI_STORE, s);
        } else {
            static const bool fp8_lnf = env_on("ME_FP8_LN_FUSE");
            const bool fuse = ln && fp8_lnf && ln_fusable(true);
            if (fuse) set_fused_layernorm(ctx, p, "vitm.ln.stats", "vitm.ln.count", *ln, ctx->cfg.ln_eps, xn, (uint8_t*)xn, xn_s);
            gemm_fp8_launch(p, EPI_RESID_SCALE, s);
            return fuse;
        }
        return false;
    }

    // vit.rs:163-170 Block::forward for the three ViTs
    void block(int i) {
        const VitBlockW &b0 = p0.blocks[i], &b1 = p1.blocks[i], &b2 = p2.blocks[i];  // by physical segment
        const int C = ctx->C(), T = ctx->T(), heads = ctx->cfg.num_heads;
        // norm2 of this block and norm1 of the next, for the residual launches that write them (resid_all, gemm8)
        const LnSet ln2{b0.ln2_w, b0.ln2_b, b1.ln2_w, b1.ln2_b, b2.ln2_w, b2.ln2_b};
        LnSet next;
        const bool has_next = i + 1 < ctx->cfg.depth;
        if (has_next) {
            const VitBlockW &n0 = p0.blocks[i + 1], &n1 = p1.blocks[i + 1], &n2 = p2.blocks[i + 1];
            next = LnSet{n0.ln1_w, n0.ln1_b, n1.ln1_w, n1.ln1_b, n2.ln1_w, n2.ln1_b};
        }
        if (ctx->fp8) {
            // BASELINE configs[3]: the linears named by me_model_config.fp8_linears (default: all four) run on the scaled
            // fp8 MFMA, each fed by a producer that writes MX fp8 -- LayerNorm (qkv, fc1), the attention kernel's own
            // store stage (proj), fc1's epilogue (fc2) -- the others on the 16-bit kernels; attention itself stays f16
            const int mask = ctx->fp8_mask;
            const bool q8 = mask & 1, p8 = mask & 2, f18 = mask & 4, f28 = mask & 8;
            const int windows = W0 + W1 * (fov ? 2 : 1);
            set_ln(b1.ln1_w, b1.ln1_b, b2.ln1_w, b2.ln1_b);
            if (q8) {
                // norm1 as MX fp8: written by the previous block's fp8 fc2 where the LayerNorm rides in its residual epilogue
                if (!xn_is_norm1_fp8)
                    layernorm_fp8_launch(tok, b0.ln1_w, b0.ln1_b, (uint8_t*)xn, xn_s, Rtot, C, ctx->cfg.ln_eps, s, &segs);
                xn_is_norm1_fp8 = false;
                gemm8(xn, xn_s, C, 3 * C, weights(i, &VitBlockW::qkv_w8, &VitBlockW::qkv_b, nullptr, &VitBlockW::qkv_ws), 0);
            } else {
                layernorm_launch(tok, b0.ln1_w, b0.ln1_b, xn, nullptr, Rtot, C, ctx->cfg.ln_eps, ctx->dtype, s, &segs);
                gemm_all(xn, C, weights(i, &VitBlockW::qkv_w, &VitBlockW::qkv_b), 3 * C, qkv, ACT_NONE, C);
            }
            if (p8) {
                // the attention kernel writes the projection's fp8 operand itself (the bytes a separate
                // quantize_f16_to_fp8 pass over its 16-bit output would give: ME_FP8_ATT_SEPARATE=1 runs that pass,
                // the test compares the two)
                static const bool separate = getenv("ME_FP8_ATT_SEPARATE") != nullptr;
                if (separate || heads % 2) {
                    attention_launch(qkv, att, windows, T, heads, ctx->dtype, s, &segs, nullptr, nullptr, 0, true);
                    quantize_f16_to_fp8_launch(att, att8, att_s, Rtot, C, 0, s);
                } else {
                    attention_launch(qkv, att, windows, T, heads, ctx->dtype, s, &segs, att8, att_s, Rtot / 128, true);
                }
                // ... and its residual epilogue norm2 as fc1's fp8 operand (the tall fp8 tile)
                const SegWeights w8 = weights(i, &VitBlockW::proj_w8, &VitBlockW::proj_b, &VitBlockW::ls1, &VitBlockW::proj_ws);
                xn_is_norm2_fp8 = gemm8(att8, att_s, C, C, w8, 3, false, f18 ? &ln2 : nullptr);
            } else {
                attention_launch(qkv, att, windows, T, heads, ctx->dtype, s, &segs, nullptr, nullptr, 0, true);
                // the 16-bit projection's residual epilogue writes norm2 as fc1's MX fp8 operand (gemm_core.h resid_ln_epilogue)
                xn_is_norm2_fp8 = resid_all(att, C, weights(i, &VitBlockW::proj_w, &VitBlockW::proj_b, &VitBlockW::ls1), f18 ? &ln2 : nullptr, true);
            }
            set_ln(b1.ln2_w, b1.ln2_b, b2.ln2_w, b2.ln2_b);
            if (f18) {
                if (!xn_is_norm2_fp8)
                    layernorm_fp8_launch(tok, b0.ln2_w, b0.ln2_b, (uint8_t*)xn, xn_s, Rtot, C, ctx->cfg.ln_eps, s, &segs);
                xn_is_norm2_fp8 = false;
                gemm8(xn, xn_s, C, 4 * C, weights(i, &VitBlockW::fc1_w8, &VitBlockW::fc1_b, nullptr, &VitBlockW::fc1_ws), 1, !f28);
            } else {
                layernorm_launch(tok, b0.ln2_w, b0.ln2_b, xn, nullptr, Rtot, C, ctx->cfg.ln_eps, ctx->dtype, s, &segs);
                gemm_all(xn, C, weights(i, &VitBlockW::fc1_w, &VitBlockW::fc1_b), 4 * C, hid, ACT_GELU);
            }
            if (f28) {
                const uint8_t* h8 = (const uint8_t*)hid;
                if (!f18) {  // a 16-bit fc1 left f16: quantised here as fc2's operand
                    uint8_t* q = (uint8_t*)site_buf(ctx, "vitm.hid8", (size_t)Rtot * 4 * C);
                    quantize_f16_to_fp8_launch(hid, q, hid_s, Rtot, 4 * C, 0, s);
                    h8 = q;
                }
                const bool fuse_next = q8 && has_next;  // the next block's qkv reads norm1 as fp8
                const SegWeights w8 = weights(i, &VitBlockW::fc2_w8, &VitBlockW::fc2_b, &VitBlockW::ls2, &VitBlockW::fc2_ws);
                xn_is_norm1_fp8 = gemm8(h8, hid_s, 4 * C, C, w8, 2, false, fuse_next ? &next : nullptr);
            } else {
                resid_all(hid, 4 * C, weights(i, &VitBlockW::fc2_w, &VitBlockW::fc2_b, &VitBlockW::ls2));
            }
            if (taps.fn) taps.fn(taps.user, i, tok + row_main * C);
            return;
        }
        // norm1: written by the previous block's fc2 launch where the LayerNorm rides in the residual epilogue
        if (!xn_is_norm1) {
            set_ln(b1.ln1_w, b1.ln1_b, b2.ln1_w, b2.ln1_b);
            layernorm_launch(tok, b0.ln1_w, b0.ln1_b, xn, nullptr, Rtot, C, ctx->cfg.ln_eps, ctx->dtype, s, &segs);
        }
        xn_is_norm1 = false;
        gemm_all(xn, C, weights(i, &VitBlockW::qkv_w, &VitBlockW::qkv_b), 3 * C, qkv, ACT_NONE, C);
        attention_launch(qkv, att, W0 + W1 * (fov ? 2 : 1), T, heads, ctx->dtype, s, &segs, nullptr, nullptr, 0, true);
        if (!resid_all(att, C, weights(i, &VitBlockW::proj_w, &VitBlockW::proj_b, &VitBlockW::ls1), &ln2)) {
            set_ln(b1.ln2_w, b1.ln2_b, b2.ln2_w, b2.ln2_b);
            layernorm_launch(tok, b0.ln2_w, b0.ln2_b, xn, nullptr, Rtot, C, ctx->cfg.ln_eps, ctx->dtype, s, &segs);
        }
        gemm_all(xn, C, weights(i, &VitBlockW::fc1_w, &VitBlockW::fc1_b), 4 * C, hid, ACT_GELU);
        xn_is_norm1 = resid_all(hid, 4 * C, weights(i, &VitBlockW::fc2_w, &VitBlockW::fc2_b, &VitBlockW::ls2), has_next ? &next : nullptr);
        if (taps.fn) taps.fn(taps.user, i, tok + row_main * C);
    }

    // vit.rs:343 final norm of each ViT; the 16-bit results of segments 0 / 1 / 2
    // want32: also keep the normalised tokens in f32 (the source of split [hi | lo] token maps)
    void finish(bool want32) {
        set_ln(p1.norm_w, p1.norm_b, p2.norm_w, p2.norm_b);
        fin32 = want32 ? (float*)site_buf(ctx, "vitm.final32", (size_t)Rtot * ctx->C() * 4) : nullptr;
        layernorm_launch(tok, p0.norm_w, p0.norm_b, fin16, fin32, Rtot, ctx->C(), ctx->cfg.ln_eps, ctx->dtype, s,
                         &segs);
    }
    // seg: 0 = patch encoder, 1 = image encoder, 2 = FOV encoder (the ViT, not the physical position)
    int64_t seg_row(int seg) const { return seg == 0 ? row_main : (seg == 1 ? row_img : row_fov); }
    void* final16(int seg) const { return fin16 + seg_row(seg) * ctx->C() * 2; }
    const float* final32(int seg) const { return fin32 + seg_row(seg) * ctx->C(); }
};
}  // namespace

void vit_forward(me_ctx* ctx, int which, const void* patches16, int W, const VitTaps& taps,
                 void* final16, float* final32, const std::string& tag, hipStream_t s) {
    VitRun run(ctx, which, patches16, W, taps, tag, s);
    for (int i = 0; i < ctx->cfg.depth; ++i) run.block(i);
    run.finish(final16, final32);
}

// encoder.rs:218-335 DepthProEncoder::forward_encodings
void stage_encoder(me_ctx* ctx, const float* img32, int B, bool with_fov) {
    stage_encoder_trunk(ctx, img32, B, with_fov);
    stage_encoder_latents(ctx, B);
}

// encoder.rs:307-309: the two latent upsample chains (taps of blocks 5 and 11 -> encodings 0 and 1).  Nothing but decoder
// levels 1 and 0 reads their results, and their ConvTranspose launches are bound by HBM writes: extract_depth_impl runs
// them beside the low-resolution decoder levels (api.hip).
void stage_encoder_latents(me_ctx* ctx, int B) {
    hipStream_t s = ctx->stream;
    const me_model_config& c = ctx->cfg;
    const int g = ctx->g(), dec = c.dec_dim, e0 = c.enc_dims[0];
    const bool sp_dec = ctx->split(SPLIT_DEC_CONVS);
    const size_t wide_dec = sp_dec ? 2 : 1;
    const int side0 = 4 * g, H0 = 32 * g, H1 = 16 * g;
    const void* lat0 = ctx->bufs.at("enc.lat0").p;
    const void* lat1 = ctx->bufs.at("enc.lat1").p;
    void* enc1 = site_buf(ctx, "enc1.16b", bordered_bytes(B, H1, H1, e0) * wide_dec);
    run_upsample(ctx, "up_latent1", lat1, B, side0, ctx->w.up_latent1, nullptr, enc1, true, 0,
                 ACT_NONE, s, sp_dec);
    // (me_ctx::enc0_sum: the f32 encoding is never formed -- decoder level 0 takes its sum with level 1's features from the
    // launch that also writes "enc0.r16b")
    float* enc0_32 = ctx->enc0_sum ? nullptr : (float*)site_buf(ctx, "enc0.f32", (size_t)B * H0 * H0 * dec * 4);
    void* enc0_r16 = site_buf(ctx, "enc0.r16b", bordered_bytes(B, H0, H0, dec));
    run_upsample(ctx, "up_latent0", lat0, B, side0, ctx->w.up_latent0, enc0_32, enc0_r16, true, 0,
                 ACT_RELU, s, false, 0, ctx->enc0_sum);
}

// [hi | lo | hi] operands of the composed ConvTransposes stored as [hi | lo], the third part read from the first
// (GemmParams::a_wrap): bit for bit the same sums.  ME_A_WRAP=0: the three parts stored.
static bool a_wrap_on() {
    static const bool on = env_on("ME_A_WRAP");
    return on;
}

// Decoder level 0 adds two maps that are each written once and read once: x1 = the last ConvTranspose of the latent0 chain and
// x0 = level 1's composed out_conv o deconv ConvTranspose, both 2x2 stride-2 over the same grid onto the same map.  Chained
// (gemm_params.h chain_convt) they are ONE accumulator over K1 + K2 and one f32 map less is written and read.  Applies to a
// whole extract_depth call when level 1 has its composed weights, the chain's last layer has the decoder's width and both
// launches would run on the 256x256 two-group tile at this shape anyway; ME_ENC0_SUM=0: the two launches.
bool enc0_sum_applies(const me_ctx* ctx, int B) {
    static const bool on = env_on("ME_ENC0_SUM");
    const UpsampleW& u = ctx->w.up_latent0;
    const FusionW& fw = ctx->w.fusions[1];
    const int dec = ctx->cfg.dec_dim, h = 16 * ctx->g();
    if (!on || !(ctx->split(SPLIT_FUSION_OUT) && fw.deconv && fw.fused_w) || u.convt.empty() || u.cout.back() != dec) return false;
    const int K1 = u.cin.back() * (ctx->split(SPLIT_UPSAMPLE) ? 2 : 1), K2 = 3 * dec;
    for (const int K : {K1, K2}) {
        const TileProblem q = {B * h * h, 4 * dec, K, 0, 0, A_PLAIN, EPI_CONVT, 0, 0, 0, h, h, 0, false, false};
        if (K % 64 || K < 128 || resolve_config(q, -1, tile_knobs()) != CFG_PP256) return false;
    }
    return true;
}

void stage_encoder_trunk(me_ctx* ctx, const float* img32, int B, bool fov_async /* = with_fov */) {
    hipStream_t s = ctx->stream;
    const me_model_config& c = ctx->cfg;
    const int g = ctx->g(), S = ctx->S(), C = ctx->C(), P = ctx->P(), T = ctx->T();
    const int dec = c.dec_dim, e1 = c.enc_dims[1], e2 = c.enc_dims[2], e3 = c.enc_dims[3];
    const bool sp = ctx->split(SPLIT_UPSAMPLE);  // merged token maps and upsample intermediates as [hi | lo]
    const bool sp_dec = ctx->split(SPLIT_DEC_CONVS);  // encodings 1..4 as [hi | lo] for decoder.convs
    const size_t wide = sp ? 2 : 1, wide_dec = sp_dec ? 2 : 1;
    report(ctx, 0.0f, "creating image pyramid");
    // encoder.rs:125-140 create_pyramid (x0 itself only changes type)
    void* x0 = site_buf(ctx, "enc.x0", (size_t)B * 3 * S * S * 2);
    void* x1 = site_buf(ctx, "enc.x1", (size_t)B * 3 * (S / 2) * (S / 2) * 2);
    void* x2 = site_buf(ctx, "enc.x2", (size_t)B * 3 * (S / 4) * (S / 4) * 2);
    cast_f32_to_16_launch(img32, x0, (int64_t)B * 3 * S * S, ctx->dtype, s);
    bilinear_launch(img32, x1, 3 * B, S, S / 2, c.align_corners, ctx->dtype, s);
    bilinear_launch(img32, x2, 3 * B, S, S / 4, c.align_corners, ctx->dtype, s);
    void* xg = site_buf(ctx, "enc.xg", (size_t)B * g * g * C * 2 * wide);
    // encoder.rs:238-250 split + cat, vit.rs:210-223 patch embed im2col
    report(ctx, 0.02f, "preparing image patches");
    void* patches = site_buf(ctx, "enc.patches", (size_t)B * 35 * P * 768 * 2);
    patchify_launch(x0, x1, x2, patches, B, g, ctx->dtype, s);

    report(ctx, 0.03f, "encoding patches");
    const int side0 = 4 * g, side1 = 2 * g;
    void* lat0 = site_buf(ctx, "enc.lat0", (size_t)B * side0 * side0 * C * 2 * wide);
    void* lat1 = site_buf(ctx, "enc.lat1", (size_t)B * side0 * side0 * C * 2 * wide);
    TapCtx tc{ctx, B, lat0, lat1, s};
    VitTaps taps;
    taps.fn = tap_fn, taps.user = &tc;
    // encoder.rs:298-303 image encoder on the 1/4 image and (fov.rs:57-63) the FOV encoder: both depend only
    // on x2; the three ViTs run as one row space on the launch stream (MergedVit above)
    void* patches2 = site_buf(ctx, "enc.patches2", (size_t)B * P * 768 * 2);
    patchify_windows_launch(x2, patches2, B, g, ctx->dtype, s);  // both small ViTs embed the same patches
    if (fov_async) report(ctx, 0.03f, "encoding fov");
    MergedVit run(ctx, B, fov_async, patches, patches2, patches2, taps, s);
    for (int i = 0; i < c.depth; ++i) run.block(i);
    run.finish(sp);
    // the final tokens feed merge: as 16-bit rows, or (split operands) as f32 rows that merge splits
    const float* tok32 = sp ? run.final32(0) : nullptr;
    const void* tok16 = sp ? nullptr : run.final16(0);
    merge_launch(sp ? run.final32(1) : nullptr, sp ? nullptr : run.final16(1), xg, B, 1, 0, 1, 0, g, C, ctx->dtype,
                 s, sp);
    if (fov_async) {
        float* lin32 = (float*)site_buf(ctx, "fov.lin", (size_t)B * T * (dec / 2) * 4);
        linear(ctx, run.final16(2), (int64_t)B * T, C, ctx->w.fov_lin_w, dec / 2, ctx->w.fov_lin_b, nullptr, lin32, ACT_NONE, s);
    }
    report(ctx, 0.55f, "reshaping patch encodings");
    // encoder.rs:263,285-294: split_with_sizes + merge
    void* x0f = site_buf(ctx, "enc.x0f", (size_t)B * side0 * side0 * C * 2 * wide);
    void* x1f = site_buf(ctx, "enc.x1f", (size_t)B * side1 * side1 * C * 2 * wide);
    void* x2f = site_buf(ctx, "enc.x2f", (size_t)B * g * g * C * 2 * wide);
    merge_launch(tok32, tok16, x0f, B, 35, 0, 5, g / 8, g, C, ctx->dtype, s, sp);
    merge_launch(tok32, tok16, x1f, B, 35, 25, 3, g / 4, g, C, ctx->dtype, s, sp);
    merge_launch(tok32, tok16, x2f, B, 35, 34, 1, 0, g, C, ctx->dtype, s, sp);

    report(ctx, 0.7f, "encoding features");
    // encoder.rs:307-316
    const int H2 = 8 * g, H3 = 4 * g, H4 = 2 * g;   // (encodings 0 and 1: stage_encoder_latents)
    void* enc2 = site_buf(ctx, "enc2.16b", bordered_bytes(B, H2, H2, e1) * wide_dec);
    run_upsample(ctx, "up0", x0f, B, side0, ctx->w.up0, nullptr, enc2, true, 0, ACT_NONE, s, sp_dec);
    void* enc3 = site_buf(ctx, "enc3.16b", bordered_bytes(B, H3, H3, e2) * wide_dec);
    run_upsample(ctx, "up1", x1f, B, side1, ctx->w.up1, nullptr, enc3, true, 0, ACT_NONE, s, sp_dec);
    // encoder.rs:316-325: upsample2, upsample_lowres, cat on channels, fuse_lowres.  Split: a pixel of `cat`
    // is [up2 hi | lowres hi | up2 lo | lowres lo], i.e. [hi(2 e3) | lo(2 e3)] against fuse_lowres' [W | W]
    char* cat = (char*)site_buf(ctx, "enc.cat", (size_t)B * H4 * H4 * 2 * e3 * 2 * wide);
    const int64_t cat_stride = 2 * e3 * (int64_t)wide;
    run_upsample(ctx, "up2", x2f, B, g, ctx->w.up2, nullptr, cat, false, cat_stride, ACT_NONE, s, sp, 2 * e3);
    report(ctx, 0.9f, "upsampling lowres");
    convt(ctx, xg, B, g, g, C, ctx->w.up_lowres_w, e3, ctx->w.up_lowres_b, nullptr, cat + (size_t)e3 * 2,
          false, cat_stride, ACT_NONE, s, sp, sp, 2 * e3);
    report(ctx, 0.95f, "fusing lowres");
    void* enc4 = site_buf(ctx, "enc4.16b", bordered_bytes(B, H4, H4, e3) * wide_dec);
    GemmParams p = linear_params((int64_t)B * H4 * H4, e3, 2 * e3, cat, ctx->w.fuse_w, ctx->w.fuse_b, enc4, nullptr);
    set_a_parts(p, (int)wide);
    set_out16_bordered(p, H4, H4);
    set_out16_parts(p, e3, (int)wide_dec);
    gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, s);
}

// the head behind head[0] as one launch on the half-resolution map (stage_head): needs the un-split chain and the 128-channel
// halo tile's shapes; ME_HEAD_COMPOSED=0: the three launches
static bool head_composed_applies(const me_ctx* ctx, int B) {
    static const bool composed_on = env_on("ME_HEAD_COMPOSED");
    const int dec = ctx->cfg.dec_dim, Hh = ctx->S() / 2;
    return composed_on && !ctx->split(SPLIT_HEAD) && ctx->w.head_fused_w && Hh % 16 == 0 && (dec / 2) % 64 == 0 &&
           ((int64_t)B * Hh * Hh) % 256 == 0;
}

// decoder.rs:153-208 MultiresConvDecoder::forward (+ :84-102 FeatureFusionBlock, :35-44 RCU)
void stage_decoder(me_ctx* ctx, int B, bool want_features32) { stage_decoder_levels(ctx, B, want_features32, 4, 0); }

void stage_decoder_levels(me_ctx* ctx, int B, bool want_features32, int first, int last) {
    hipStream_t s = ctx->stream;
    const me_model_config& c = ctx->cfg;
    const int g = ctx->g(), dec = c.dec_dim;
    const int H[5] = {32 * g, 16 * g, 8 * g, 4 * g, 2 * g};
    const int Cin[5] = {dec, c.enc_dims[0], c.enc_dims[1], c.enc_dims[2], c.enc_dims[3]};
    const char* enc_names[5] = {"enc0.r16b", "enc1.16b", "enc2.16b", "enc3.16b", "enc4.16b"};

    const bool sp_dec = ctx->split(SPLIT_DEC_CONVS), spf = ctx->split(SPLIT_FUSION_OUT),
               sp_head = ctx->split(SPLIT_HEAD);
    // `features` carried between levels (f32 residual path): the level above left them in its ".feat.f32" buffer
    float* feat32 = first == 4 ? nullptr : (float*)ctx->bufs.at("dec" + std::to_string(first + 1) + ".feat.f32").p;
    for (int i = first; i >= last; --i) {
        report(ctx, (4 - i) / 5.0f, i == 4 ? "decoding initial block" : "decoding blocks");
        const std::string L = "dec" + std::to_string(i);
        const int h = H[i];
        const size_t n32 = (size_t)B * h * h * dec * 4, nb = bordered_bytes(B, h, h, dec);
        const FusionW& fw = ctx->w.fusions[i];
        const void* enc = ctx->bufs.at(enc_names[i]).p;

        // features_i = convs[i-1](encoding) (3x3, no bias); level 0 uses the encoding as is
        float* x1_32;
        void* x1_r16;
        if (i == 0 && ctx->enc0_sum) {
            // x0 + x1 from one launch: the latent0 chain's last ConvTranspose (its ReLU'd bordered 16-bit output from the
            // accumulators after its own K loop) and level 1's composed one on top, + out_conv's bias
            const UpsampleW& u = ctx->w.up_latent0;
            const FusionW& f1 = ctx->w.fusions[1];
            ME_CHECK(ctx->enc0_last_in && ctx->enc0_last_side * 2 == h, ME_ERR_BAD_ARG, "decoder: the latent0 chain left no operand for level 0");
            x1_32 = (float*)site_buf(ctx, "dec0.x01.f32", n32);
            x1_r16 = (void*)enc;
            feat32 = nullptr;
            const GemmParams first = convt_params(ctx->enc0_last_in, B, h / 2, h / 2, u.cin.back(), u.convt.back(), dec, nullptr, nullptr, x1_r16,
                                                  true, 0, ACT_RELU, ctx->split(SPLIT_UPSAMPLE));
            const GemmParams second = convt_params(ctx->bufs.at("dec1.v16").p, B, h / 2, h / 2, dec, f1.fused_w, dec, f1.out_b, nullptr, nullptr,
                                                   false, 0, ACT_NONE, false, false, 0, 3, a_wrap_on());
            GemmParams p = chain_convt(first, second, x1_32);
            p.grid_cap = ctx->grid_cap;
            gemm_launch(p, A_PLAIN, EPI_CONVT, ctx->dtype, s, CFG_PP256);
        } else if (i == 0) {
            x1_32 = (float*)ctx->bufs.at("enc0.f32").p;
            x1_r16 = (void*)enc;
        } else {
            // level 4's conv output is `lowres_features` (decoder.rs:178), kept for the FOV head
            x1_32 = (float*)site_buf(ctx, i == 4 ? std::string("lowres.f32") : L + ".x1.f32", n32);
            x1_r16 = site_buf(ctx, L + ".x1.r16b", nb);
            ConvOut o;
            o.out32 = x1_32, o.out16 = x1_r16, o.border16 = true, o.act = ACT_RELU;
            conv(ctx, enc, B, h, h, Cin[i], ctx->w.dec_convs[i], dec, 3, 1, nullptr, o, s, sp_dec);
        }

        float* out32;
        void* out_r16;
        if (i == 4) {
            // decoder.rs:171-183: lowres_features = features.clone(); fusions.last()(features, None)
            out32 = x1_32;
            out_r16 = x1_r16;
        } else {
            // out = x0 + resnet1(x1) = x0 + x1 + conv2(relu(conv1(relu(x1))))
            void* t_r16 = site_buf(ctx, L + ".t1.r16b", nb);
            ConvOut o1;
            o1.out16 = t_r16, o1.border16 = true, o1.act = ACT_RELU;
            conv(ctx, x1_r16, B, h, h, dec, fw.resnet1.w[0], dec, 3, 1, fw.resnet1.b[0], o1, s);
            out32 = (float*)site_buf(ctx, L + ".out.f32", n32);
            out_r16 = site_buf(ctx, L + ".out.r16b", nb);
            ConvOut o2;
            o2.out32 = out32, o2.out16 = out_r16, o2.border16 = true, o2.act = ACT_RELU;
            o2.res32 = x1_32, o2.res32b = feat32;
            conv(ctx, t_r16, B, h, h, dec, fw.resnet1.w[1], dec, 3, 1, fw.resnet1.b[1], o2, s);
        }
        // resnet2
        void* t2_r16 = site_buf(ctx, L + ".t2.r16b", nb);
        ConvOut o3;
        o3.out16 = t2_r16, o3.border16 = true, o3.act = ACT_RELU;
        conv(ctx, out_r16, B, h, h, dec, fw.resnet2.w[0], dec, 3, 1, fw.resnet2.b[0], o3, s);
        // the operands of deconv and out_conv have no residual path beside them: [hi | lo] under SPLIT_FUSION_OUT,
        // [hi | lo | hi] where the two are composed into one ConvTranspose (FusionW::fused_w)
        const bool fused = spf && fw.deconv && fw.fused_w;
        const bool wrap = fused && a_wrap_on();  // [hi | lo | hi] stored as [hi | lo]
        const size_t wf = fused && !wrap ? 3 : (spf ? 2 : 1);
        if (i == 0) {
            // decoder.rs:101 out_conv + mod.rs:326 head[0] as ONE convolution (weights.hip compose_features): this level's last
            // convolution writes out_conv's INPUT as head[0]'s zero-bordered operand, the 1x1 launch and the feature map between
            // them (0.9 GB of traffic at 768 x 768) go.  Not when the caller wants the features themselves, nor under SPLIT_HEAD;
            // ME_FEAT_COMPOSED=0: the two layers as they are.
            static const bool feat_composed_on = env_on("ME_FEAT_COMPOSED");
            ctx->features_pre = feat_composed_on && !want_features32 && head_composed_applies(ctx, B) && ctx->w.feat_fused_w;
            if (ctx->features_pre) {
                ConvOut o4;
                o4.out16 = site_buf(ctx, "features.16b", bordered_bytes(B, h, h, dec)), o4.border16 = true, o4.res32 = out32;
                conv(ctx, t2_r16, B, h, h, dec, fw.resnet2.w[1], dec, 3, 1, fw.resnet2.b[1], o4, s);
                continue;
            }
        }
        void* v16 = site_buf(ctx, L + ".v16", (size_t)B * h * h * dec * 2 * wf);
        ConvOut o4;
        o4.out16 = v16, o4.res32 = out32, o4.parts16 = (int)wf;
        conv(ctx, t2_r16, B, h, h, dec, fw.resnet2.w[1], dec, 3, 1, fw.resnet2.b[1], o4, s);
        if (fused) {
            // (me_ctx::enc0_sum: level 0's chained launch reads this level's "dec1.v16" itself)
            if (i == 1 && ctx->enc0_sum) continue;
            // out_conv(deconv(v)) as ONE launch: f32 features of the next level straight from the pixel shuffle
            const int64_t Mo = (int64_t)B * 4 * h * h;
            feat32 = (float*)site_buf(ctx, L + ".feat.f32", (size_t)Mo * dec * 4);
            convt(ctx, v16, B, h, h, dec, fw.fused_w, dec, fw.out_b, feat32, nullptr, false, 0, ACT_NONE, s, false, false,
                  0, 3, wrap);
            continue;
        }
        // deconv (levels 1-4) then out_conv 1x1 (+bias)
        const void* pre = v16;
        int ho = h;
        if (fw.deconv) {
            void* d16 = site_buf(ctx, L + ".d16", (size_t)B * 4 * h * h * dec * 2 * wf);
            convt(ctx, v16, B, h, h, dec, fw.deconv, dec, nullptr, nullptr, d16, false, 0, ACT_NONE, s, spf, spf);
            pre = d16, ho = 2 * h;
        }
        const int64_t Mo = (int64_t)B * ho * ho;
        if (i > 0) {
            feat32 = (float*)site_buf(ctx, L + ".feat.f32", (size_t)Mo * dec * 4);
            linear(ctx, pre, Mo, dec, fw.out_w, dec, fw.out_b, nullptr, feat32, ACT_NONE, s, spf);
        } else {
            // final features: 16-bit zero-bordered operand of head[0]; f32 copy for the ABI
            float* f32 = want_features32 ? (float*)site_buf(ctx, "features.f32", (size_t)Mo * dec * 4)
                                         : nullptr;
            void* f16b = site_buf(ctx, "features.16b", bordered_bytes(B, ho, ho, dec) * (sp_head ? 2 : 1));
            GemmParams p = linear_params(Mo, dec, dec, pre, fw.out_w, fw.out_b, f16b, f32);
            set_a_parts(p, (int)wf);
            set_out16_bordered(p, ho, ho);
            set_out16_parts(p, dec, sp_head ? 2 : 1);
            gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, s);
        }
    }
}

// mod.rs:323-333 head convs + ReLUs, mod.rs:361-362 div_scalar + clamp fused into the last kernel
// pre_image: "features.16b" holds the input of the last fusion block's out_conv instead of its output (ctx->features_pre)
void stage_head(me_ctx* ctx, int B, const float* f_norm_dev, bool clamp, float* depth_dev, bool pre_image) {
    hipStream_t s = ctx->stream;
    const me_model_config& c = ctx->cfg;
    const int dec = c.dec_dim, S = ctx->S(), Hh = S / 2;
    report(ctx, 0.0f, "forwarding head");
    // mod.rs:323-333 is one chain without a residual path: its operands are [hi | lo] under SPLIT_HEAD
    const bool sp = ctx->split(SPLIT_HEAD);
    const size_t wide = sp ? 2 : 1;
    const void* f16b = ctx->bufs.at("features.16b").p;
    const float clamp_lo = clamp ? 1e-4f : -INFINITY, clamp_hi = clamp ? 1e4f : INFINITY;  // mod.rs:362
    // mod.rs:326-333 behind head[0]: ConvTranspose -> conv3x3 -> ReLU -> conv1x1 -> ReLU as ONE launch on the half-resolution map,
    // the two linear layers composed at load time (weights.hip compose_head): the [B, 128, 1536, 1536] tensor between them (605 MB
    // written and read back) never exists.  Needs the un-split chain and the 128-channel halo tile's shapes; ME_HEAD_COMPOSED=0:
    // the three launches below.
    ME_CHECK(!pre_image || head_composed_applies(ctx, B), ME_ERR_BAD_ARG, "head: composed features without the composed head");
    if (head_composed_applies(ctx, B)) {
        void* h0b = site_buf(ctx, "head.h0b", bordered_bytes(B, Hh, Hh, dec / 2));
        ConvOut o;
        o.out16 = h0b, o.border16 = true;
        if (pre_image) {
            o.tap_bias = ctx->w.feat_fused_b + dec / 2;
            conv(ctx, f16b, B, Hh, Hh, dec, ctx->w.feat_fused_w, dec / 2, 3, 1, ctx->w.feat_fused_b, o, s, false);
        } else {
            conv(ctx, f16b, B, Hh, Hh, dec, ctx->w.head0_w, dec / 2, 3, 1, ctx->w.head0_b, o, s, false);
        }
        // head_fused_b: the bias [32], its per-tap shares [9][32], and head.4.weight as the 32 floats the epilogue reads
        // (compose_head pads the head_dims[0] of the checkpoint with zeros)
        const float* fb = ctx->w.head_fused_b;
        head_composed_launch(head_composed_params(h0b, B, Hh, Hh, dec / 2, ctx->w.head_fused_w, fb, fb + 32, fb + 32 + 9 * 32,
                                                  ctx->w.head4_b, f_norm_dev, clamp_lo, clamp_hi, depth_dev),
                             ctx->dtype, s);
        return;
    }
    void* h0 = site_buf(ctx, "head.h0", (size_t)B * Hh * Hh * (dec / 2) * 2 * wide);
    ConvOut o;
    o.out16 = h0, o.parts16 = (int)wide;
    conv(ctx, f16b, B, Hh, Hh, dec, ctx->w.head0_w, dec / 2, 3, 1, ctx->w.head0_b, o, s, sp);
    void* h1 = site_buf(ctx, "head.h1b", bordered_bytes(B, S, S, dec / 2) * wide);
    convt(ctx, h0, B, Hh, Hh, dec / 2, ctx->w.head1_w, dec / 2, ctx->w.head1_b, nullptr, h1, true, 0,
          ACT_NONE, s, sp, sp);
    gemm_launch(head_final_params(h1, B, S, S, dec / 2, ctx->w.head2_w, c.head_dims[0], ctx->w.head2_b, ctx->w.head4_w, ctx->w.head4_b,
                                  f_norm_dev, clamp_lo, clamp_hi, depth_dev, sp),
                A_CONV, EPI_HEAD_FINAL, ctx->dtype, s);
}

// fov.rs:40-63: the FOV encoder (third ViT-L on "enc.x2", the 1/4 image) and its Linear
void stage_fov_vit(me_ctx* ctx, int B, hipStream_t s) {
    const int g = ctx->g(), C = ctx->C(), P = ctx->P(), T = ctx->T(), dec = ctx->cfg.dec_dim;
    report(ctx, 0.0f, "encoding fov");
    const void* x2 = ctx->bufs.at("enc.x2").p;
    void* patches = site_buf(ctx, "fov.patches", (size_t)B * P * 768 * 2);
    patchify_windows_launch(x2, patches, B, g, ctx->dtype, s);
    void* tok16 = site_buf(ctx, "fov.tok16", (size_t)B * T * C * 2);
    vit_forward(ctx, ME_VIT_FOV_ENCODER, patches, B, VitTaps(), tok16, nullptr, "vit.fov", s);
    float* lin32 = (float*)site_buf(ctx, "fov.lin", (size_t)B * T * (dec / 2) * 4);
    linear(ctx, tok16, (int64_t)B * T, C, ctx->w.fov_lin_w, dec / 2, ctx->w.fov_lin_b, nullptr, lin32, ACT_NONE, s);
}

// fov.rs:66-88: the convolutional tail; needs "fov.lin" (stage_fov_vit) and "lowres.f32" (decoder)
void stage_fov_tail(me_ctx* ctx, int B, float* fov_deg_dev) {
    hipStream_t s = ctx->stream;
    const me_model_config& c = ctx->cfg;
    const int g = ctx->g(), P = ctx->P(), T = ctx->T(), dec = c.dec_dim;
    report(ctx, 0.85f, "fov lowres");
    const float* lin32 = (const float*)ctx->bufs.at("fov.lin").p;
    // fov.rs:70-74: relu(downsample[0](lowres)) + reshaped tokens
    const float* low32 = (const float*)ctx->bufs.at("lowres.f32").p;
    void* low16b = site_buf(ctx, "fov.low16b", bordered_bytes(B, 2 * g, 2 * g, dec));
    nhwc32_to_16b_launch(low32, low16b, B, 2 * g, 2 * g, dec, 0, ctx->dtype, s);
    float* fl32 = (float*)site_buf(ctx, "fov.down", (size_t)B * P * (dec / 2) * 4);
    ConvOut o0;
    o0.out32 = fl32, o0.act = ACT_RELU, o0.act16_only = false;
    conv(ctx, low16b, B, 2 * g, 2 * g, dec, ctx->w.fov_down_w, dec / 2, 3, 2, ctx->w.fov_down_b, o0, s);
    void* fx = site_buf(ctx, "fov.x16b", bordered_bytes(B, g, g, dec / 2));
    fov_add_relu_launch(lin32, fl32, fx, B, g, dec / 2, T, ctx->dtype, s);
    // fov.rs:77-85 head
    void* f1 = site_buf(ctx, "fov.h0b", bordered_bytes(B, g / 2, g / 2, dec / 4));
    ConvOut o1;
    o1.out16 = f1, o1.border16 = true, o1.act = ACT_RELU;
    conv(ctx, fx, B, g, g, dec / 2, ctx->w.fov_h0_w, dec / 4, 3, 2, ctx->w.fov_h0_b, o1, s);
    void* f2 = site_buf(ctx, "fov.h2", (size_t)B * (g / 4) * (g / 4) * (dec / 8) * 2);
    ConvOut o2;
    o2.out16 = f2, o2.act = ACT_RELU;
    conv(ctx, f1, B, g / 2, g / 2, dec / 4, ctx->w.fov_h2_w, dec / 8, 3, 2, ctx->w.fov_h2_b, o2, s);
    float* fnorm = (float*)site_buf(ctx, "f_norm", (size_t)B * 4);
    fov_final_launch(f2, ctx->w.fov_h4_w, ctx->w.fov_h4_b, fov_deg_dev, fnorm, B, g / 4, dec / 8,
                     ctx->dtype, s);
}

}  // namespace me
