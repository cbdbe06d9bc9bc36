// extern "C" boundary of libmatrixeyes_hip.so (include/matrix_eyes_hip.h, matrix_eyes_hip_ops.h).
// Every entry point converts internal me::Error into a status code + last_error text (model.h
// ME_API_BEGIN / ME_API_END); nothing throws or aborts across the boundary.  The clamp, raster and file
// entries of the output back end are in output_api.hip, its mesh entries in mesh_writer.hip (the write-behind
// ones in file_write.hip), the photo-input entries in input_api.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "../../include/matrix_eyes_hip_ops.h"
#include "model.h"

#include "admission.h"
#include "mx_fp8.h"

using namespace me;

// (admission.h states the act rules of the entries in Act: the ABI's values are the same)
static_assert((int)ME_ACT_NONE == ACT_NONE && (int)ME_ACT_GELU == ACT_GELU && (int)ME_ACT_RELU == ACT_RELU, "ME_ACT_* are Act");

namespace {

thread_local std::string g_create_error;

void check_ready(me_ctx* ctx) {
    ME_CHECK(ctx->finalized, ME_ERR_NOT_READY,
             "weights are not finalized (me_weights_finalize / me_bcast_weights)");
}

void check_batch(int32_t batch) {
    ME_CHECK(batch >= 1 && batch <= 64, ME_ERR_BAD_SHAPE, "batch %d out of range [1, 64]", batch);
}

void validate_config(const me_model_config& c) {
    ME_CHECK(c.grid >= 8 && c.grid % 8 == 0 && c.grid <= 64, ME_ERR_BAD_SHAPE,
             "grid %d: need a multiple of 8 in [8, 64]", c.grid);
    ME_CHECK(c.embed_dim == 64 * c.num_heads && c.num_heads >= 1, ME_ERR_BAD_SHAPE,
             "embed_dim %d must be 64 * num_heads (%d)", c.embed_dim, c.num_heads);
    ME_CHECK(c.embed_dim == 64 || c.embed_dim == 128 || c.embed_dim == 256 || c.embed_dim == 512 ||
                 c.embed_dim == 1024,
             ME_ERR_BAD_SHAPE, "embed_dim %d not in {64,128,256,512,1024}", c.embed_dim);
    ME_CHECK(c.depth >= 1 && c.depth <= 64, ME_ERR_BAD_SHAPE, "depth %d", c.depth);
    // vit.rs:318-324: a requested tap that does not exist panics
    ME_CHECK(c.tap_blocks[0] >= 0 && c.tap_blocks[0] < c.depth && c.tap_blocks[1] >= 0 &&
                 c.tap_blocks[1] < c.depth && c.tap_blocks[0] != c.tap_blocks[1],
             ME_ERR_BAD_SHAPE, "tap blocks {%d,%d} with depth %d", c.tap_blocks[0], c.tap_blocks[1],
             c.depth);
    for (int i = 0; i < 4; ++i)
        ME_CHECK(c.enc_dims[i] > 0 && c.enc_dims[i] % 64 == 0, ME_ERR_BAD_SHAPE,
                 "enc_dims[%d] = %d must be a multiple of 64", i, c.enc_dims[i]);
    ME_CHECK(c.dec_dim > 0 && c.dec_dim % 256 == 0, ME_ERR_BAD_SHAPE,
             "dec_dim %d must be a multiple of 256", c.dec_dim);
    ME_CHECK(c.head_dims[0] > 0 && c.head_dims[0] <= 32 && c.head_dims[0] % 4 == 0 &&
                 c.head_dims[1] == 1,
             ME_ERR_BAD_SHAPE, "head_dims {%d,%d}: need {<=32 multiple of 4, 1}", c.head_dims[0],
             c.head_dims[1]);
    ME_CHECK(c.ln_eps > 0.f, ME_ERR_BAD_ARG, "ln_eps %g", (double)c.ln_eps);
    ME_CHECK(c.split_operands >= 0 && c.split_operands <= 15, ME_ERR_BAD_ARG, "split_operands %d not in [0, 15]",
             c.split_operands);
}

}  // namespace

namespace {
__global__ void status_clear_bits_kernel(unsigned* word, unsigned bits) { atomicAnd(word, ~bits); }

// The fused residual + LayerNorm launch gave up waiting for a sibling workgroup (another tenant on the device's CUs, a
// CU mask the runtime does not report): from here on this context runs the stand-alone LayerNorm launches.  Logged once.
void latch_ln_fallback(me_ctx* ctx, const char* where) {
    if (ctx->ln_fuse_off) return;
    ctx->ln_fuse_off = true;
    ctx->drop_graph();  // the captured step holds the fused launches
    ctx->ln_fuse_note = std::string("LayerNorm fusion switched off for this context (") + where +
                        "): a workgroup of the fused residual + LayerNorm launch gave up waiting for its row tile's other "
                        "column tiles -- the device's CUs are shared or masked.  The stand-alone LayerNorm launches run from "
                        "here on (the ME_LN_FUSE=0 results, bit for bit)";
    fprintf(stderr, "matrix-eyes-hip: %s\n", ctx->ln_fuse_note.c_str());
}

// What earlier ASYNCHRONOUS steps (device results) raised, as far as their closing copy of the status word into the
// pinned mirror has landed -- no synchronisation.  A timed-out exchange means those steps' depth maps are invalid: the
// entry that finds it out fails (so that a caller who never polls me_status_flags still gets an error), with fusion
// off and the bit cleared, so the call can simply be made again.
void check_pending_status(me_ctx* ctx) {
    if (!ctx->status_host) return;
    const unsigned pending = *ctx->status_host;
    if (!(pending & ME_STATUS_SYNC_TIMEOUT)) return;
    latch_ln_fallback(ctx, "found at the next entry into the library");
    hipLaunchKernelGGL(status_clear_bits_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->status_dev, (unsigned)ME_STATUS_SYNC_TIMEOUT);
    ME_HIP(hipGetLastError());
    ME_HIP(hipStreamSynchronize(ctx->stream));
    *ctx->status_host = pending & ~(unsigned)ME_STATUS_SYNC_TIMEOUT;
    fail(ME_ERR_HIP,
         "an earlier asynchronous me_extract_depth step timed out in the fused LayerNorm exchange (ME_STATUS_SYNC_TIMEOUT): its "
         "depth map is not valid.  LayerNorm fusion is now off for this context; submit the work again");
}
}  // namespace

namespace me {
std::string& create_error() { return g_create_error; }

OutBuf out_buf(me_ctx* ctx, void* user, size_t bytes, const std::string& name) {
    OutBuf o;
    o.user = user, o.bytes = bytes;
    if (is_device_ptr(user)) {
        o.dev = user;
    } else {
        o.dev = site_buf(ctx, name, bytes);
        o.staged = true;
    }
    return o;
}

void finish(me_ctx* ctx, const OutBuf& o) {
    if (o.staged) from_device(ctx, o.user, o.dev, o.bytes);
}

void check_resize_shape(const char* who, int32_t w, int32_t h, int32_t nw, int32_t nh) {
    ME_CHECK(w > 0 && h > 0 && nw > 0 && nh > 0, ME_ERR_BAD_SHAPE, "%s: %dx%d -> %dx%d", who, w, h, nw, nh);
    ME_CHECK(w <= ME_RESIZE_MAX_DIM && h <= ME_RESIZE_MAX_DIM && nw <= ME_RESIZE_MAX_DIM && nh <= ME_RESIZE_MAX_DIM,
             ME_ERR_BAD_SHAPE, "%s: %dx%d -> %dx%d: a side exceeds ME_RESIZE_MAX_DIM (%d)", who, w, h, nw, nh,
             ME_RESIZE_MAX_DIM);
}

namespace {
me_ctx::DepthSlot* find_depth_slot(me_ctx* ctx, const void* p) {
    const char* q = (const char*)p;
    for (me_ctx::DepthSlot& s : ctx->depth_slots)
        if (s.base && q >= s.base && q < s.base + s.bytes) return &s;
    return nullptr;
}
}  // namespace

OutputScope::OutputScope(me_ctx* c, const void* depth) : ctx(c) {
    if (!c->output_overlap || !c->out_stream || c->capturing) return;
    saved = c->stream;
    me_ctx::DepthSlot* s = depth && is_device_ptr(depth) ? find_depth_slot(c, depth) : nullptr;
    if (s && s->has_produced) {
        ME_HIP(hipStreamWaitEvent(c->out_stream, s->produced, 0));
        slot = (int)(s - c->depth_slots);
    } else {
        // a buffer no step of this context has written (a caller's own depth, a host pointer): behind everything queued so far
        hipEvent_t ev = nullptr;
        ME_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        const hipError_t e1 = hipEventRecord(ev, saved), e2 = e1 == hipSuccess ? hipStreamWaitEvent(c->out_stream, ev, 0) : e1;
        (void)hipEventDestroy(ev);  // (released once it has completed)
        ME_HIP(e2);
    }
    c->stream = c->out_stream;
    active = true;
}
OutputScope::~OutputScope() {
    if (!active) return;
    if (slot >= 0) {
        me_ctx::DepthSlot& s = ctx->depth_slots[slot];
        if (!s.consumed && hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming) != hipSuccess) s.consumed = nullptr;
        if (s.consumed && hipEventRecord(s.consumed, ctx->out_stream) == hipSuccess) s.has_consumed = true;
    }
    ctx->stream = saved;
}
}  // namespace me

namespace {
// the step that is about to write [out, out + bytes): behind every output call that still reads an overlapping buffer
void wait_for_consumers(me_ctx* ctx, const void* out, size_t bytes) {
    if (!ctx->output_overlap) return;
    const char* lo = (const char*)out;
    for (me_ctx::DepthSlot& s : ctx->depth_slots)
        if (s.base && s.has_consumed && lo < s.base + s.bytes && s.base < lo + bytes) {
            ME_HIP(hipStreamWaitEvent(ctx->stream, s.consumed, 0));
            s.has_consumed = false;
        }
}
// ... and, once it is queued, known as the producer of that range
void mark_produced(me_ctx* ctx, const void* out, size_t bytes) {
    if (!ctx->output_overlap) return;
    me_ctx::DepthSlot* slot = nullptr;
    for (me_ctx::DepthSlot& s : ctx->depth_slots)
        if (s.base == (const char*)out) slot = &s;
    if (!slot)
        for (me_ctx::DepthSlot& s : ctx->depth_slots)
            if (!s.base) {
                slot = &s;
                break;
            }
    if (!slot) {
        slot = &ctx->depth_slots[0];
        for (me_ctx::DepthSlot& s : ctx->depth_slots)   // the least recently produced
            if (s.stamp < slot->stamp) slot = &s;
    }
    if (slot->base != (const char*)out && slot->has_consumed) {
        // the range this slot stood for is forgotten: nothing may still be reading it unordered
        ME_HIP(hipStreamWaitEvent(ctx->stream, slot->consumed, 0));
        slot->has_consumed = false;
    }
    if (!slot->produced) ME_HIP(hipEventCreateWithFlags(&slot->produced, hipEventDisableTiming));
    slot->base = (const char*)out, slot->bytes = bytes, slot->stamp = ++ctx->depth_stamp;
    ME_HIP(hipEventRecord(slot->produced, ctx->stream));
    slot->has_produced = true;
}
}  // namespace

extern "C" {

int32_t me_abi_version(void) { return ME_ABI_VERSION; }

int32_t me_default_config(me_model_config* cfg) {
    if (!cfg) return ME_ERR_BAD_ARG;
    // vit.rs:17-19,349-358; encoder.rs:227; mod.rs:262-263,308-311
    cfg->grid = 24, cfg->embed_dim = 1024, cfg->num_heads = 16, cfg->depth = 24;
    cfg->tap_blocks[0] = 5, cfg->tap_blocks[1] = 11;
    cfg->enc_dims[0] = 256, cfg->enc_dims[1] = 512, cfg->enc_dims[2] = 1024, cfg->enc_dims[3] = 1024;
    cfg->dec_dim = 256;
    cfg->head_dims[0] = 32, cfg->head_dims[1] = 1;
    cfg->ln_eps = 1e-5f;
    cfg->align_corners = 1;
    cfg->split_operands = 3;
    cfg->fp8_linears = 0;
    return ME_OK;
}

int32_t me_ctx_create(int32_t device_id, int32_t dtype, const me_model_config* cfg, me_ctx** out) {
    if (!out) return ME_ERR_BAD_ARG;
    *out = nullptr;
    me_ctx* ctx = nullptr;
    try {
        ME_CHECK(dtype == ME_DTYPE_F16 || dtype == ME_DTYPE_BF16 || dtype == ME_DTYPE_FP8, ME_ERR_BAD_ARG,
                 "bad dtype %d", dtype);
        int ndev = 0;
        const hipError_t e = hipGetDeviceCount(&ndev);
        ME_CHECK(e == hipSuccess && ndev > 0, ME_ERR_HIP,
                 "no HIP device available (%s): this library has no CPU fallback",
                 e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        ME_CHECK(device_id >= 0 && device_id < ndev, ME_ERR_BAD_ARG, "device %d of %d", device_id,
                 ndev);
        ctx = new me_ctx();
        ctx->device = device_id;
        // fp8 contexts: every 16-bit operand is f16 (the checkpoint's own type), the big ViT linears are MX fp8
        ctx->fp8 = dtype == ME_DTYPE_FP8;
        ctx->dtype = ctx->fp8 ? ME_DTYPE_F16 : dtype;
        if (cfg)
            ctx->cfg = *cfg;
        else
            me_default_config(&ctx->cfg);
        // diagnostic override of the DEFAULT split_operands (tools/split_budget.py).  A caller-supplied
        // configuration is never overridden: the mask fixes the arena layout, which ranks that exchange arenas
        // must agree on (me_bcast_weights compares me_ctx::arena_layout_hash)
        if (const char* e = getenv("ME_SPLIT_OPERANDS")) {
            if (!cfg) ctx->cfg.split_operands = atoi(e);
            else if (atoi(e) != cfg->split_operands)
                fprintf(stderr, "matrix-eyes-hip: ME_SPLIT_OPERANDS=%s ignored, the caller's me_model_config says %d\n", e,
                        cfg->split_operands);
        }
        if (const char* e = getenv("ME_GRAPH")) ctx->graph_enabled = atoi(e) != 0;
        validate_config(ctx->cfg);
        ME_CHECK(!ctx->fp8 || ctx->cfg.embed_dim % 256 == 0, ME_ERR_BAD_SHAPE,
                 "ME_DTYPE_FP8 needs embed_dim a multiple of 256 (256x256 tiles, K slabs of 128): %d", ctx->cfg.embed_dim);
        ctx->split_mask = ctx->cfg.split_operands;  // model.h SplitStage bits
        if (const char* e = getenv("ME_FP8_LINEARS")) {     // diagnostic override of the default (tools/fp8_budget.py)
            if (!cfg || cfg->fp8_linears == 0) ctx->cfg.fp8_linears = atoi(e);
        }
        ME_CHECK(ctx->cfg.fp8_linears >= 0 && ctx->cfg.fp8_linears <= 15, ME_ERR_BAD_ARG, "fp8_linears %d not in [0, 15]",
                 ctx->cfg.fp8_linears);
        ctx->fp8_mask = ctx->fp8 ? (ctx->cfg.fp8_linears ? ctx->cfg.fp8_linears : ME_FP8_LINEARS_DEFAULT) : 0;
        ME_HIP(hipSetDevice(device_id));
        ME_HIP(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
        ctx->stream = ctx->own_stream;
        ME_HIP(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
        {
            // the output stream's launches are few and short (0.7 ms of kernels per image beside a 22 ms depth step): at the
            // highest priority they take the first CUs a boundary of the main stream's persistent kernels frees, and the host
            // thread that waits for their counts and copies waits less
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (hipStreamCreateWithPriority(&ctx->out_stream, hipStreamNonBlocking, greatest) != hipSuccess) {
                (void)hipGetLastError();
                ME_HIP(hipStreamCreateWithFlags(&ctx->out_stream, hipStreamNonBlocking));
            }
        }
        ME_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        ME_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        ME_HIP(hipMalloc((void**)&ctx->status_dev, 256));
        ME_HIP(hipMemset(ctx->status_dev, 0, 256));
        ME_HIP(hipHostMalloc((void**)&ctx->status_host, 64, hipHostMallocDefault));
        *ctx->status_host = 0;
        build_weight_table(ctx);
        ME_HIP(hipMalloc((void**)&ctx->arena, ctx->arena_bytes));
        // the alignment gaps between slots belong to the arena's bytes (the cache file, its checksum, a broadcast): zero, not whatever
        // the allocation held
        ME_HIP(hipMemset(ctx->arena, 0, ctx->arena_bytes));
        resolve_weights(ctx);
        *out = ctx;
        return ME_OK;
    } catch (const me::Error& e) {
        g_create_error = e.msg;
        if (ctx) me_ctx_destroy(ctx);
        return e.code;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        if (ctx) me_ctx_destroy(ctx);
        return ME_ERR_BAD_ARG;
    }
}

void me_ctx_destroy(me_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);
    if (ctx->out_stream) (void)hipStreamSynchronize(ctx->out_stream);
    ctx->drop_graph();
    // the status word of this context may be the calling thread's current one (ME_API_BEGIN): not after this
    if (me::current_status_word() == ctx->status_dev) me::set_current_status_word(nullptr);
    for (auto& kv : ctx->bufs)
        if (kv.second.p) (void)hipFree(kv.second.p);
    me::free_resample_tables(ctx);
    me::free_jpeg_scratch(ctx);
    me::free_png_scratch(ctx);
    me::free_stereogram_noise_scratch(ctx);
    me::free_weight_pack(ctx);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->arena8) (void)hipFree(ctx->arena8);
    if (ctx->status_dev) (void)hipFree(ctx->status_dev);
    if (ctx->status_host) (void)hipHostFree((void*)ctx->status_host);
    (void)me_output_flush(ctx);  // pending write-behind files are completed before their buffers go
    for (me_ctx::WriteSlot& w : ctx->write_slots)
        if (w.pinned) (void)hipHostFree(w.pinned);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->out_stream) (void)hipStreamDestroy(ctx->out_stream);
    for (me_ctx::DepthSlot& d : ctx->depth_slots) {
        if (d.produced) (void)hipEventDestroy(d.produced);
        if (d.consumed) (void)hipEventDestroy(d.consumed);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char* me_last_error(const me_ctx* ctx) {
    return ctx ? ctx->last_error.c_str() : g_create_error.c_str();
}

int32_t me_ctx_set_progress(me_ctx* ctx, me_progress_fn fn, void* user) {
    if (!ctx) return ME_ERR_BAD_ARG;
    ctx->progress = fn, ctx->progress_user = user;
    return ME_OK;
}

int32_t me_ctx_set_stream(me_ctx* ctx, void* hip_stream) {
    ME_API_BEGIN(ctx)
    ME_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    ctx->drop_graph();
    ME_API_END(ctx)
}

int32_t me_ctx_synchronize(me_ctx* ctx) {
    ME_API_BEGIN(ctx)
    ME_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->output_overlap && ctx->out_stream) ME_HIP(hipStreamSynchronize(ctx->out_stream));
    ME_API_END(ctx)
}

int32_t me_ctx_set_output_overlap(me_ctx* ctx, int32_t on) {
    ME_API_BEGIN(ctx)
    ME_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->out_stream) ME_HIP(hipStreamSynchronize(ctx->out_stream));
    ctx->output_overlap = on != 0 && ctx->out_stream != nullptr;
    for (me_ctx::DepthSlot& d : ctx->depth_slots) d.base = nullptr, d.bytes = 0, d.has_produced = d.has_consumed = false;
    ME_API_END(ctx)
}

// ---- weights ----------------------------------------------------------------------------
int32_t me_load_weight(me_ctx* ctx, const char* name, const void* data, int32_t weight_dtype,
                       const int64_t* dims, int32_t ndim) {
    ME_API_BEGIN(ctx)
    load_weight(ctx, name, data, weight_dtype, dims, ndim);
    ME_API_END(ctx)
}

int32_t me_expected_weight_count(const me_ctx* ctx) { return ctx ? (int32_t)ctx->slots.size() : 0; }

int32_t me_expected_weight(const me_ctx* ctx, int32_t index, const char** name, int64_t dims[4],
                           int32_t* ndim) {
    if (!ctx || index < 0 || index >= (int32_t)ctx->slots.size() || !name || !dims || !ndim)
        return ME_ERR_BAD_ARG;
    const WeightSlot& s = ctx->slots[index];
    *name = s.name.c_str();
    *ndim = (int32_t)s.dims.size();
    for (int i = 0; i < 4; ++i) dims[i] = i < *ndim ? s.dims[i] : 1;
    return ME_OK;
}

int32_t me_weights_finalize(me_ctx* ctx) {
    ME_API_BEGIN(ctx)
    finalize_weights(ctx);
    ME_API_END(ctx)
}

int32_t me_load_checkpoint_pt(me_ctx* ctx, const char* path) {
    ME_API_BEGIN(ctx)
    load_checkpoint_pt(ctx, path);
    ME_API_END(ctx)
}

int32_t me_unused_weight_count(const me_ctx* ctx) { return ctx ? (int32_t)ctx->unused_weights.size() : 0; }

const char* me_unused_weight_name(const me_ctx* ctx, int32_t index) {
    if (!ctx || index < 0 || index >= (int32_t)ctx->unused_weights.size()) return nullptr;
    return ctx->unused_weights[index].c_str();
}

int64_t me_weight_arena_bytes(const me_ctx* ctx) { return ctx ? (int64_t)ctx->arena_bytes : 0; }

uint64_t me_weight_arena_layout(const me_ctx* ctx) { return ctx ? ctx->arena_layout_hash() : 0; }

int32_t me_status_flags(me_ctx* ctx, uint32_t* flags) {
    ME_API_BEGIN(ctx)
    ME_CHECK(flags, ME_ERR_BAD_ARG, "me_status_flags: null pointer");
    uint32_t host = 0;
    ME_HIP(hipMemcpyAsync(&host, ctx->status_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    ME_HIP(hipMemsetAsync(ctx->status_dev, 0, 4, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    *ctx->status_host = 0;
    // the steps that raised it are lost (the caller knows: the bit is in *flags); the ones after this call are not
    if (host & ME_STATUS_SYNC_TIMEOUT) latch_ln_fallback(ctx, "me_status_flags saw ME_STATUS_SYNC_TIMEOUT");
    *flags = host;
    ME_API_END(ctx)
}

int32_t me_calibrate(me_ctx* ctx, double* out6) {
    ME_API_BEGIN(ctx)
    ME_CHECK(out6, ME_ERR_BAD_ARG, "me_calibrate: null pointer");
    calibrate(ctx, out6);
    ME_API_END(ctx)
}

int32_t me_ln_fusion_state(me_ctx* ctx, int32_t* fused, int32_t* fallbacks) {
    if (!ctx) return ME_ERR_BAD_ARG;
    if (fused) *fused = ctx->ln_fuse_off ? 0 : 1;
    if (fallbacks) *fallbacks = ctx->ln_fallbacks;
    return ME_OK;
}

void* me_weight_arena_ptr(const me_ctx* ctx) { return ctx ? (void*)ctx->arena : nullptr; }

int32_t me_weights_adopt(me_ctx* ctx) {
    ME_API_BEGIN(ctx)
    adopt_weights(ctx);
    ME_API_END(ctx)
}

// ---- forward passes ----------------------------------------------------------------------
int32_t me_preprocess_u8(me_ctx* ctx, const uint8_t* rgb, int32_t batch, float* img) {
    ME_API_BEGIN(ctx)
    ME_CHECK(rgb && img, ME_ERR_BAD_ARG, "me_preprocess_u8: null pointer");
    check_batch(batch);
    const int S = ctx->S();
    const size_t npix = (size_t)batch * S * S;
    const void* src = to_device(ctx, rgb, npix * 3, "io.rgb");
    OutBuf o = out_buf(ctx, img, npix * 3 * 4, "io.img");
    preprocess_u8_launch((const uint8_t*)src, (float*)o.dev, batch, S, ctx->stream);
    finish(ctx, o);
    ME_API_END(ctx)
}

namespace {
struct ApiTap {
    me_ctx* ctx;
    const int32_t* blocks;
    int n;
    float** dev;
    size_t bytes;
};
void api_tap_fn(void* user, int index, const float* tokens) {
    ApiTap* t = (ApiTap*)user;
    for (int i = 0; i < t->n; ++i)
        if (t->blocks[i] == index)
            ME_HIP(hipMemcpyAsync(t->dev[i], tokens, t->bytes, hipMemcpyDeviceToDevice,
                                  t->ctx->stream));
}
}  // namespace

int32_t me_vit_forward_features(me_ctx* ctx, int32_t which_vit, const float* xs, int32_t windows,
                                const int32_t* intermediate_blocks, int32_t n_intermediate,
                                float* final_out, float* const* intermediate_out) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    ME_CHECK(which_vit >= 0 && which_vit <= 2, ME_ERR_BAD_ARG, "which_vit %d", which_vit);
    ME_CHECK(xs && final_out, ME_ERR_BAD_ARG, "me_vit_forward_features: null pointer");
    ME_CHECK(windows >= 1 && windows <= 4096, ME_ERR_BAD_SHAPE, "windows %d", windows);
    ME_CHECK(n_intermediate >= 0 && n_intermediate <= 8 &&
                 (n_intermediate == 0 || (intermediate_blocks && intermediate_out)),
             ME_ERR_BAD_ARG, "bad intermediate block list");
    for (int i = 0; i < n_intermediate; ++i)  // vit.rs:318-324 "only {} / {} blocks found"
        ME_CHECK(intermediate_blocks[i] >= 0 && intermediate_blocks[i] < ctx->cfg.depth,
                 ME_ERR_BAD_SHAPE, "only %d blocks, block %d requested", ctx->cfg.depth,
                 intermediate_blocks[i]);
    const int g = ctx->g(), P = ctx->P(), T = ctx->T(), C = ctx->C(), win = 16 * g;
    const size_t in_elems = (size_t)windows * 3 * win * win;
    const float* xs_dev = (const float*)to_device(ctx, xs, in_elems * 4, "api.vit.in");
    void* xs16 = site_buf(ctx, "api.vit.in16", in_elems * 2);
    cast_f32_to_16_launch(xs_dev, xs16, (int64_t)in_elems, ctx->dtype, ctx->stream);
    void* patches = site_buf(ctx, "api.vit.patches", (size_t)windows * P * 768 * 2);
    patchify_windows_launch(xs16, patches, windows, g, ctx->dtype, ctx->stream);
    const size_t tok_bytes = (size_t)windows * T * C * 4;
    std::vector<OutBuf> inter(n_intermediate);
    std::vector<float*> inter_dev(n_intermediate);
    for (int i = 0; i < n_intermediate; ++i) {
        ME_CHECK(intermediate_out[i], ME_ERR_BAD_ARG, "null intermediate output %d", i);
        inter[i] = out_buf(ctx, intermediate_out[i], tok_bytes, "api.vit.inter" + std::to_string(i));
        inter_dev[i] = (float*)inter[i].dev;
    }
    ApiTap tap{ctx, intermediate_blocks, n_intermediate, inter_dev.data(), tok_bytes};
    VitTaps taps;
    if (n_intermediate) taps.fn = api_tap_fn, taps.user = &tap;
    OutBuf fin = out_buf(ctx, final_out, tok_bytes, "api.vit.final");
    vit_forward(ctx, which_vit, patches, windows, taps, nullptr, (float*)fin.dev, "vit.api",
                ctx->stream);
    finish(ctx, fin);
    for (auto& o : inter) finish(ctx, o);
    ME_API_END(ctx)
}

int32_t me_encoder_forward_encodings(me_ctx* ctx, const float* x, int32_t batch,
                                     float* const encodings[5]) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    check_batch(batch);
    ME_CHECK(x && encodings, ME_ERR_BAD_ARG, "me_encoder_forward_encodings: null pointer");
    for (int i = 0; i < 5; ++i) ME_CHECK(encodings[i], ME_ERR_BAD_ARG, "null encoding %d", i);
    const me_model_config& c = ctx->cfg;
    const int S = ctx->S(), g = ctx->g();
    const float* x_dev = (const float*)to_device(ctx, x, (size_t)batch * 3 * S * S * 4, "io.img");
    stage_encoder(ctx, x_dev, batch, false);
    const int H[5] = {32 * g, 16 * g, 8 * g, 4 * g, 2 * g};
    const int Cc[5] = {c.dec_dim, c.enc_dims[0], c.enc_dims[1], c.enc_dims[2], c.enc_dims[3]};
    const char* names[5] = {"enc0.f32", "enc1.16b", "enc2.16b", "enc3.16b", "enc4.16b"};
    for (int i = 0; i < 5; ++i) {
        OutBuf o = out_buf(ctx, encodings[i], (size_t)batch * Cc[i] * H[i] * H[i] * 4,
                           "api.enc.out" + std::to_string(i));
        if (i == 0)
            nhwc32_to_nchw32_launch((const float*)ctx->bufs.at(names[i]).p, (float*)o.dev, batch, H[i],
                                    H[i], Cc[i], ctx->stream);
        else
            nhwc16_to_nchw32_launch(ctx->bufs.at(names[i]).p, (float*)o.dev, batch, H[i], H[i], Cc[i],
                                    1, ctx->dtype, ctx->stream, ctx->split(SPLIT_DEC_CONVS));
        finish(ctx, o);
    }
    ME_API_END(ctx)
}

int32_t me_decoder_forward(me_ctx* ctx, const float* const encodings[5], int32_t batch,
                           float* features, float* lowres_features) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    check_batch(batch);
    ME_CHECK(encodings && features && lowres_features, ME_ERR_BAD_ARG,
             "me_decoder_forward: null pointer");
    const me_model_config& c = ctx->cfg;
    const int g = ctx->g(), dec = c.dec_dim;
    const int H[5] = {32 * g, 16 * g, 8 * g, 4 * g, 2 * g};
    const int Cc[5] = {dec, c.enc_dims[0], c.enc_dims[1], c.enc_dims[2], c.enc_dims[3]};
    const char* names[5] = {"enc0.r16b", "enc1.16b", "enc2.16b", "enc3.16b", "enc4.16b"};
    for (int i = 0; i < 5; ++i) {
        ME_CHECK(encodings[i], ME_ERR_BAD_ARG, "null encoding %d", i);
        const size_t n = (size_t)batch * Cc[i] * H[i] * H[i];
        const float* src =
            (const float*)to_device(ctx, encodings[i], n * 4, "api.dec.in" + std::to_string(i));
        const bool sp = i > 0 && ctx->split(SPLIT_DEC_CONVS);  // encoding 0 only feeds the residual units
        void* d16 = site_buf(ctx, names[i], (size_t)batch * (H[i] + 2) * (H[i] + 2) * Cc[i] * 2 * (sp ? 2 : 1));
        float* d32 = i == 0 ? (float*)site_buf(ctx, "enc0.f32", n * 4) : nullptr;
        nchw32_to_nhwc_launch(src, d32, d16, batch, H[i], H[i], Cc[i], 1, i == 0 ? 1 : 0, ctx->dtype,
                              ctx->stream, sp);
    }
    stage_decoder(ctx, batch, true);
    OutBuf of = out_buf(ctx, features, (size_t)batch * dec * H[0] * H[0] * 4, "api.dec.feat");
    nhwc32_to_nchw32_launch((const float*)ctx->bufs.at("features.f32").p, (float*)of.dev, batch, H[0],
                            H[0], dec, ctx->stream);
    finish(ctx, of);
    OutBuf ol = out_buf(ctx, lowres_features, (size_t)batch * dec * H[4] * H[4] * 4, "api.dec.low");
    nhwc32_to_nchw32_launch((const float*)ctx->bufs.at("lowres.f32").p, (float*)ol.dev, batch, H[4],
                            H[4], dec, ctx->stream);
    finish(ctx, ol);
    ME_API_END(ctx)
}

int32_t me_head_forward(me_ctx* ctx, const float* features, int32_t batch,
                        float* canonical_inverse_depth) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    check_batch(batch);
    ME_CHECK(features && canonical_inverse_depth, ME_ERR_BAD_ARG, "me_head_forward: null pointer");
    const int S = ctx->S(), Hh = S / 2, dec = ctx->cfg.dec_dim;
    const size_t n = (size_t)batch * dec * Hh * Hh;
    const float* src = (const float*)to_device(ctx, features, n * 4, "api.head.in");
    const bool sp = ctx->split(SPLIT_HEAD);
    void* f16b = site_buf(ctx, "features.16b", (size_t)batch * (Hh + 2) * (Hh + 2) * dec * 2 * (sp ? 2 : 1));
    nchw32_to_nhwc_launch(src, nullptr, f16b, batch, Hh, Hh, dec, 1, 0, ctx->dtype, ctx->stream, sp);
    OutBuf o = out_buf(ctx, canonical_inverse_depth, (size_t)batch * S * S * 4, "io.depth");
    stage_head(ctx, batch, nullptr, false, (float*)o.dev);
    finish(ctx, o);
    ME_API_END(ctx)
}

int32_t me_fov_forward(me_ctx* ctx, const float* x, const float* lowres_feature, int32_t batch,
                       float* fov_deg) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    check_batch(batch);
    ME_CHECK(x && lowres_feature && fov_deg, ME_ERR_BAD_ARG, "me_fov_forward: null pointer");
    const int S = ctx->S(), g = ctx->g(), dec = ctx->cfg.dec_dim;
    const float* x_dev = (const float*)to_device(ctx, x, (size_t)batch * 3 * S * S * 4, "io.img");
    void* x2 = site_buf(ctx, "enc.x2", (size_t)batch * 3 * (S / 4) * (S / 4) * 2);
    bilinear_launch(x_dev, x2, 3 * batch, S, S / 4, ctx->cfg.align_corners, ctx->dtype, ctx->stream);
    const size_t nl = (size_t)batch * dec * 4 * g * g;
    const float* low = (const float*)to_device(ctx, lowres_feature, nl * 4, "api.fov.low");
    float* low32 = (float*)site_buf(ctx, "lowres.f32", nl * 4);
    nchw32_to_nhwc_launch(low, low32, nullptr, batch, 2 * g, 2 * g, dec, 0, 0, ctx->dtype, ctx->stream);
    OutBuf o = out_buf(ctx, fov_deg, (size_t)batch * 4, "fov_deg");
    stage_fov_vit(ctx, batch, ctx->stream);
    stage_fov_tail(ctx, batch, (float*)o.dev);
    finish(ctx, o);
    ME_API_END(ctx)
}

namespace {
// the range a stage reports into, restored on scope exit (also when a stage throws)
struct ProgressRange {
    me_ctx* ctx;
    ProgressRange(me_ctx* c, float lo, float hi) : ctx(c) { ctx->prog_lo = lo, ctx->prog_hi = hi; }
    ~ProgressRange() { ctx->prog_lo = 0.0f, ctx->prog_hi = 1.0f; }
};

void extract_depth_impl(me_ctx* ctx, const float* img_dev, int32_t batch, const float* f_norm,
                        float* inverse_depth, float* fov_deg_out) {
    const int S = ctx->S();
    // mod.rs:265-293,345: the reference splits its progress bar 80 / 20 between depth and FOV when the FOV
    // head runs, the depth part 80 / 20 between encoder and the rest, that 98 / 2 between decoder and head,
    // and gives the first 5 % of each part to loading its weights (resident here).  The FOV tail runs
    // before the head in this pipeline (f_norm is divided out inside the head's last kernel), so it takes
    // the range between decoder and head.
    const float depth_end = f_norm ? 1.0f : 0.8f;
    const float enc_end = 0.8f * depth_end, dec_end = enc_end + 0.98f * (depth_end - enc_end);
    const float head_lo = f_norm ? dec_end : 0.99f;
    // Side branch (model.h me_ctx::side_stream).  The decoder's levels 4 - 2 and the FOV tail are 40 launches of 15 - 130 us
    // on 144 - 576 workgroups each -- latency-bound, most of the chip idle -- and depend only on encodings 2 - 4; the
    // encoder's two latent chains (encodings 1 and 0, read by levels 1 and 0 only) are ConvTranspose launches bound by
    // their HBM writes.  The two run side by side: fork behind the encoder trunk, join in front of level 1; the
    // persistent launches of the main branch leave half of the CUs to the side branch meanwhile.  Same kernels, same
    // order per buffer: the depth is bit for bit that of the one-stream order.  What it buys is small -- 22.84 -> 22.74 ms
    // per step (profiles/r04_side_stream.txt): side by side the ConvTranspose launch takes 404 us instead of 242 and the
    // small convolutions beside it three times their own time; both are short of memory-system bandwidth, not of CUs.
    // OFF by default since round 5 (VERDICT r4 weak 14 / ADVICE r4): 0.1 ms is inside the box-to-box noise, the small
    // launches themselves get slower beside the ConvTranspose, and the forked region adds a failure mode to graph capture
    // (a CaptureAbort between fork and join leaves the side stream attached to the aborted capture until EndCapture returns
    // Unjoined).  ME_OVERLAP_TAIL=1 switches it on for the A/B.
    static const bool overlap_env = env_flag("ME_OVERLAP_TAIL");
    const bool overlap = overlap_env && ctx->overlap_tail && ctx->side_stream && !ctx->progress && !profiler().enabled;
    // the whole path, nobody asks for encoding 0 or level 1's features themselves: decoder level 0 may take their sum from one
    // chained ConvTranspose launch (pipeline.hip enc0_sum_applies); the stage-wise entries never see the flag set
    struct Enc0Sum {
        me_ctx* c;
        ~Enc0Sum() { c->enc0_sum = false, c->enc0_last_in = nullptr; }
    } enc0_sum{ctx};
    ctx->enc0_sum = enc0_sum_applies(ctx, batch);
    OutBuf ofov;
    if (overlap) {
        stage_encoder_trunk(ctx, img_dev, batch, f_norm == nullptr);
        // (the stages below call site_buf behind the fork too -- first call only; that is safe because hipMalloc / hipFree
        // synchronise the whole device, not because the buffers exist beforehand)
        hipStream_t main_stream = ctx->stream;
        struct Restore {
            me_ctx* c;
            hipStream_t s;
            ~Restore() { c->stream = s, c->grid_cap = 0; }
        } restore{ctx, main_stream};
        if (!f_norm) ofov = out_buf(ctx, fov_deg_out ? fov_deg_out : nullptr, (size_t)batch * 4, "fov_deg");
        ME_HIP(hipEventRecord(ctx->ev_fork, main_stream));
        ME_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
        ctx->stream = ctx->side_stream;
        stage_decoder_levels(ctx, batch, false, 4, 4);
        if (!f_norm) stage_fov_tail(ctx, batch, (float*)ofov.dev);   // needs level 4's lowres features only
        stage_decoder_levels(ctx, batch, false, 3, 2);
        ME_HIP(hipEventRecord(ctx->ev_join, ctx->side_stream));
        ctx->stream = main_stream;
        static const int cap = env_int("ME_OVERLAP_CAP", 128);
        ctx->grid_cap = cap;
        stage_encoder_latents(ctx, batch);
        ctx->grid_cap = 0;
        ME_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
        ++ctx->side_branch_steps;
        stage_decoder_levels(ctx, batch, false, 1, 0);
    } else {
        {
            ProgressRange r(ctx, 0.05f * enc_end, enc_end);
            stage_encoder(ctx, img_dev, batch, f_norm == nullptr);
        }
        {
            ProgressRange r(ctx, enc_end + 0.05f * (dec_end - enc_end), dec_end);
            stage_decoder(ctx, batch, false);
        }
    }
    float* fnorm_dev = (float*)site_buf(ctx, "f_norm", (size_t)batch * 4);
    if (f_norm) {
        if (is_device_ptr(f_norm))
            ME_HIP(hipMemcpyAsync(fnorm_dev, f_norm, (size_t)batch * 4, hipMemcpyDeviceToDevice,
                                  ctx->stream));
        else
            ME_HIP(hipMemcpyAsync(fnorm_dev, f_norm, (size_t)batch * 4, hipMemcpyHostToDevice,
                                  ctx->stream));
    } else if (!overlap) {
        // mod.rs:343-358
        ofov = out_buf(ctx, fov_deg_out ? fov_deg_out : nullptr, (size_t)batch * 4, "fov_deg");
        ProgressRange r(ctx, dec_end, head_lo);
        stage_fov_tail(ctx, batch, (float*)ofov.dev);
    }
    OutBuf o = out_buf(ctx, inverse_depth, (size_t)batch * S * S * 4, "io.depth");
    {
        ProgressRange r(ctx, head_lo, 1.0f);
        stage_head(ctx, batch, fnorm_dev, true, (float*)o.dev, ctx->features_pre);
    }
    finish(ctx, o);
    if (!f_norm && fov_deg_out) finish(ctx, ofov);
    report(ctx, 1.0f, nullptr);
}

// The overflow guard of a call that hands its result to the host (the stream has been synchronised by then): the
// reference computes in f32 and has no 65504 limit (decoder.rs:35-44), so an f16 operand that left the range is an
// error of THIS back end, reported instead of a silently zeroed conv branch.
// Returns true when the step must be run again: its fused LayerNorm exchange timed out (the context has fallen back to
// the stand-alone launches by then).  Only the bit that is reported is cleared: an overflow raised beside
// a timeout, or by an earlier asynchronous step, is still there for the re-run's own check / me_status_flags.
bool settle_host_result(me_ctx* ctx, bool may_rerun) {
    uint32_t host = 0;
    ME_HIP(hipMemcpy(&host, ctx->status_dev, 4, hipMemcpyDeviceToHost));
    auto clear = [&](unsigned bits) {
        hipLaunchKernelGGL(status_clear_bits_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->status_dev, bits);
        ME_HIP(hipGetLastError());
        ME_HIP(hipStreamSynchronize(ctx->stream));
        *ctx->status_host &= ~bits;
    };
    if (host & ME_STATUS_SYNC_TIMEOUT) {
        clear(ME_STATUS_SYNC_TIMEOUT);
        if (may_rerun && !ctx->ln_fuse_off) {
            latch_ln_fallback(ctx, "the step is being run again");
            ++ctx->ln_fallbacks;
            return true;
        }
        fail(ME_ERR_HIP,
             "a workgroup of the fused residual + LayerNorm launch gave up waiting for its neighbours' statistics (another "
             "process holding the device's CUs?): the depth map is not valid.  ME_LN_FUSE=0 runs the LayerNorm as its own launch");
    }
    if (host & ME_STATUS_OVERFLOW_16BIT) {
        clear(ME_STATUS_OVERFLOW_16BIT);
        fail(ME_ERR_OVERFLOW,
             "an activation left the f16 operand range (|x| > 65504) and was stored as +-inf: the depth map is not the "
             "reference's.  Create the context with ME_DTYPE_BF16 for this checkpoint");
    }
    return false;
}

// One step = preprocess (u8 entry) + extract_depth_impl, enqueued on ctx->stream.
void enqueue_step(me_ctx* ctx, int entry, const void* in_dev, int32_t batch, const float* f_norm,
                  float* inverse_depth, float* fov_deg_out) {
    const int S = ctx->S();
    // The status word is STICKY: nothing clears it when a step starts.  A call whose result goes to the host reports what
    // it finds when it has finished (settle_host_result: its own flags and whatever earlier asynchronous steps left
    // unread -- reporting those late beats erasing them) and clears the bit it reports; with a device result only
    // me_status_flags reads and clears, so that a loop of asynchronous calls (bench.py, a captured graph's replays) cannot
    // lose the overflow of an earlier step.
    const float* img_dev = (const float*)in_dev;
    if (entry == 1) {
        float* img = (float*)site_buf(ctx, "io.img", (size_t)batch * S * S * 3 * 4);
        preprocess_u8_launch((const uint8_t*)in_dev, img, batch, S, ctx->stream);
        img_dev = img;
    }
    extract_depth_impl(ctx, img_dev, batch, f_norm, inverse_depth, fov_deg_out);
    // a device result is asynchronous: leave the status word where the next entry finds it without synchronising
    if (is_device_ptr(inverse_depth))
        ME_HIP(hipMemcpyAsync((void*)ctx->status_host, ctx->status_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
}

// The step through a hipGraph when nothing in it needs the host: every pointer on the device, no progress
// callback, no per-kernel timing.  First sight of a key: eager (allocates every site buffer); second: captured
// and instantiated; later: one hipGraphLaunch.  A capture that cannot complete (a buffer would have to grow, the
// runtime refuses a call) is discarded and the key stays eager.
void run_step(me_ctx* ctx, int entry, const void* in_dev, int32_t batch, const float* f_norm,
              float* inverse_depth, float* fov_deg_out) {
    const bool eligible = ctx->graph_enabled && !ctx->progress && !profiler().enabled && is_device_ptr(inverse_depth) &&
                          (!f_norm || is_device_ptr(f_norm)) && (f_norm || !fov_deg_out || is_device_ptr(fov_deg_out));
    if (!eligible) {
        enqueue_step(ctx, entry, in_dev, batch, f_norm, inverse_depth, fov_deg_out);
        return;
    }
    me_ctx::GraphKey key;
    key.in = in_dev, key.f_norm = f_norm, key.depth = inverse_depth, key.fov = f_norm ? nullptr : fov_deg_out;
    key.stream = ctx->stream, key.batch = batch, key.entry = entry, key.weights_generation = ctx->weights_generation;
    if (!(ctx->graph_seen && ctx->graph_key == key)) {
        ctx->drop_graph();
        ctx->graph_key = key, ctx->graph_seen = true;
        enqueue_step(ctx, entry, in_dev, batch, f_norm, inverse_depth, fov_deg_out);
        return;
    }
    if (!ctx->graph_exec && !ctx->graph_refused) {
        hipGraph_t graph = nullptr;
        bool ok = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed) == hipSuccess;
        if (ok) {
            ctx->capturing = true;
            try {
                enqueue_step(ctx, entry, in_dev, batch, f_norm, inverse_depth, fov_deg_out);
            } catch (...) {
                ok = false;
            }
            ctx->capturing = false;
            if (hipStreamEndCapture(ctx->stream, &graph) != hipSuccess) ok = false;
        }
        if (ok && graph && hipGraphInstantiate(&ctx->graph_exec, graph, nullptr, nullptr, 0) != hipSuccess)
            ctx->graph_exec = nullptr;
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        if (!ctx->graph_exec) ctx->graph_refused = true;
    }
    if (ctx->graph_exec) {
        ME_HIP(hipGraphLaunch(ctx->graph_exec, ctx->stream));
        ++ctx->graph_launches;
    } else {
        enqueue_step(ctx, entry, in_dev, batch, f_norm, inverse_depth, fov_deg_out);
    }
}
}  // namespace

int32_t me_extract_depth(me_ctx* ctx, const float* img, int32_t batch, const float* f_norm,
                         float* inverse_depth, float* fov_deg_out) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    check_batch(batch);
    ME_CHECK(img && inverse_depth, ME_ERR_BAD_ARG, "me_extract_depth: null pointer");
    const int S = ctx->S();
    check_pending_status(ctx);
    const bool in_dev = is_device_ptr(img);
    const float* img_dev = (const float*)to_device(ctx, img, (size_t)batch * 3 * S * S * 4, "io.img");
    const size_t depth_bytes = (size_t)batch * S * S * 4;
    if (is_device_ptr(inverse_depth)) wait_for_consumers(ctx, inverse_depth, depth_bytes);
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (in_dev)
            run_step(ctx, 0, img_dev, batch, f_norm, inverse_depth, fov_deg_out);
        else
            enqueue_step(ctx, 0, img_dev, batch, f_norm, inverse_depth, fov_deg_out);
        // a device result is asynchronous (me_status_flags / the next entry's check_pending_status); a host result is
        // checked here, and a step whose fused LayerNorm exchange timed out is run once more without the fusion
        if (is_device_ptr(inverse_depth) || !settle_host_result(ctx, attempt == 0)) break;
    }
    if (is_device_ptr(inverse_depth)) mark_produced(ctx, inverse_depth, depth_bytes);
    ME_API_END(ctx)
}

int32_t me_extract_depth_u8(me_ctx* ctx, const uint8_t* rgb, int32_t batch, const float* f_norm,
                            float* inverse_depth, float* fov_deg_out) {
    ME_API_BEGIN(ctx)
    check_ready(ctx);
    check_batch(batch);
    ME_CHECK(rgb && inverse_depth, ME_ERR_BAD_ARG, "me_extract_depth_u8: null pointer");
    const int S = ctx->S();
    const size_t npix = (size_t)batch * S * S;
    check_pending_status(ctx);
    const bool in_dev = is_device_ptr(rgb);
    const void* src = to_device(ctx, rgb, npix * 3, "io.rgb");
    const size_t depth_bytes = (size_t)batch * S * S * 4;
    if (is_device_ptr(inverse_depth)) wait_for_consumers(ctx, inverse_depth, depth_bytes);
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (in_dev)
            run_step(ctx, 1, src, batch, f_norm, inverse_depth, fov_deg_out);
        else
            enqueue_step(ctx, 1, src, batch, f_norm, inverse_depth, fov_deg_out);
        if (is_device_ptr(inverse_depth) || !settle_host_result(ctx, attempt == 0)) break;
    }
    if (is_device_ptr(inverse_depth)) mark_produced(ctx, inverse_depth, depth_bytes);
    ME_API_END(ctx)
}

int32_t me_ctx_set_graph(me_ctx* ctx, int32_t on) {
    ME_API_BEGIN(ctx)
    ctx->graph_enabled = on != 0;
    if (!on) ctx->drop_graph();
    ME_API_END(ctx)
}
int64_t me_graph_launch_count(const me_ctx* ctx) { return ctx ? ctx->graph_launches : 0; }
int64_t me_side_branch_count(const me_ctx* ctx) { return ctx ? ctx->side_branch_steps : 0; }

// ---- kernel-level surface (matrix_eyes_hip_ops.h) -------------------------------------------
static unsigned long long* g_stamps = nullptr;  // diagnostic builds (-DME_GEMM_STAMPS) only
extern "C" int32_t me_debug_set_stamps(void* dev_ptr) {
    g_stamps = (unsigned long long*)dev_ptr;
    return ME_OK;
}

int32_t me_op_linear(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, const void* W16,
                     const float* bias, void* out16, float* out32, int32_t act, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    GemmParams p = linear_params(M, N, K, A16, W16, bias, out16, out32, act);
    p.stamps = g_stamps;
    gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_linear_residual(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16,
                              const void* W16, const float* bias, const float* gamma, float* x32,
                              int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(bias && gamma && x32, ME_ERR_BAD_ARG, "me_op_linear_residual: null pointer");
    GemmParams p = resid_params(M, N, K, A16, W16, bias, gamma, x32);
    p.stamps = g_stamps;
    gemm_launch(p, A_PLAIN, EPI_RESID_SCALE, ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_attention(me_ctx* ctx, const void* qkv16, void* out16, int32_t windows, int32_t tokens,
                        int32_t heads) {
    ME_API_BEGIN(ctx)
    ME_CHECK(qkv16 && out16, ME_ERR_BAD_ARG, "me_op_attention: null pointer");
    attention_launch(qkv16, out16, windows, tokens, heads, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_attention_prescaled(me_ctx* ctx, const void* qkv16, void* out16, int32_t windows, int32_t tokens,
                                  int32_t heads) {
    ME_API_BEGIN(ctx)
    ME_CHECK(qkv16 && out16, ME_ERR_BAD_ARG, "me_op_attention_prescaled: null pointer");
    attention_launch(qkv16, out16, windows, tokens, heads, ctx->dtype, ctx->stream, nullptr, nullptr, nullptr, 0, true);
    ME_API_END(ctx)
}

int32_t me_op_linear_scaled_cols(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, const void* W16,
                                 const float* bias, void* out16, int32_t qcols, float qscale, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(A16 && W16 && bias && out16, ME_ERR_BAD_ARG, "me_op_linear_scaled_cols: null pointer");
    GemmParams p = linear_params(M, N, K, A16, W16, bias, out16, nullptr);
    set_scaled_cols(p, qcols, qscale);
    gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_layernorm(me_ctx* ctx, const float* x32, const float* weight, const float* bias,
                        void* y16, float* y32, int64_t rows, int32_t dim, float eps) {
    ME_API_BEGIN(ctx)
    ME_CHECK(x32 && weight && bias && (y16 || y32), ME_ERR_BAD_ARG, "me_op_layernorm: null pointer");
    layernorm_launch(x32, weight, bias, y16, y32, rows, dim, eps, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

// me_op_conv2d and me_op_conv2d_forms: the pipeline's conv() with the tile the caller names
static void conv2d_launch(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* w16, int32_t Cout,
                          int32_t k, int32_t stride, const float* bias, const float* res32, const float* res32b, float* out32,
                          void* out16, int32_t border16, int32_t out16_parts, int32_t act, int32_t act_both, int32_t tile_cfg) {
    ConvOut o;
    o.out32 = out32, o.out16 = out16, o.border16 = border16 != 0, o.parts16 = out16_parts, o.act = act, o.act16_only = !act_both;
    o.res32 = res32, o.res32b = res32b;
    gemm_launch(conv_params(in16b, B, H, W, Cin, w16, Cout, k, stride, bias, o), A_CONV, EPI_STORE, ctx->dtype, ctx->stream, tile_cfg);
}

int32_t me_op_conv2d(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin,
                     const void* w16, int32_t Cout, int32_t k, int32_t stride, const float* bias,
                     const float* res32, const float* res32b, float* out32, void* out16,
                     int32_t border16, int32_t act, int32_t act_both, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    admit_op_conv2d(k, stride);
    conv2d_launch(ctx, in16b, B, H, W, Cin, w16, Cout, k, stride, bias, res32, res32b, out32, out16, border16, 1, act, act_both, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_head_final(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* w16,
                         int32_t Cmid, const float* bias, const float* w2, const float* b2, const float* f_norm,
                         float clamp_lo, float clamp_hi, float* out32, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(in16b && w16 && bias && w2 && b2 && out32, ME_ERR_BAD_ARG, "me_op_head_final: null pointer");
    admit_op_head_final(B, H, W, Cin, Cmid);
    gemm_launch(head_final_params(in16b, B, H, W, Cin, w16, Cmid, bias, w2, b2, f_norm, clamp_lo, clamp_hi, out32), A_CONV, EPI_HEAD_FINAL,
                ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_conv_transpose2x2(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                int32_t Cin, const void* w16, int32_t Cout, const float* bias,
                                float* out32, void* out16, int32_t border16, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    gemm_launch(convt_params(in16, B, H, W, Cin, w16, Cout, bias, out32, out16, border16 != 0, 0, ACT_NONE), A_PLAIN, EPI_CONVT, ctx->dtype,
                ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

// ---- the split-operand output forms: the descriptors of pipeline.hip's conv / linear / convt helpers (gemm_params.h), the same code ----
int32_t me_op_conv2d_forms(me_ctx* ctx, const void* in16b, int32_t B, int32_t H, int32_t W, int32_t Cin,
                           const void* w16, int32_t Cout, int32_t k, int32_t stride, const float* bias,
                           const float* res32, const float* res32b, float* out32, void* out16,
                           int32_t border16, int32_t out16_parts, int32_t act, int32_t act_both, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(in16b && w16 && (out32 || out16), ME_ERR_BAD_ARG, "me_op_conv2d_forms: null pointer");
    admit_op_conv2d_forms(B, H, W, Cin, Cout, k, stride, out16, out16_parts, act);
    conv2d_launch(ctx, in16b, B, H, W, Cin, w16, Cout, k, stride, bias, res32, res32b, out32, out16, border16, out16_parts, act, act_both,
                  tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_linear_split(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, const void* W16,
                           const float* bias, void* out16, float* out32, int32_t act, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(A16 && W16 && out16, ME_ERR_BAD_ARG, "me_op_linear_split: null pointer");
    GemmParams p = linear_params(M, N, K, A16, W16, bias, out16, out32, act);
    set_out16_parts(p, N, 2);
    gemm_launch(p, A_PLAIN, EPI_STORE, ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

static void conv_transpose2x2_forms(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                    int32_t Cin, int32_t a_wrap, const void* w16, int32_t Cout, const float* bias,
                                    float* out32, void* out16, int32_t border16, int32_t act16,
                                    int32_t out_split, int32_t pixel_stride, int32_t lo_off, int32_t tile_cfg) {
    ME_CHECK(in16 && w16 && (out32 || out16), ME_ERR_BAD_ARG, "me_op_conv_transpose2x2_forms: null pointer");
    admit_op_conv_transpose2x2_forms(B, H, W, Cin, a_wrap, Cout, out16, act16, out_split, pixel_stride, lo_off);
    GemmParams p = convt_params(in16, B, H, W, Cin, w16, Cout, bias, out32, out16, border16 != 0, pixel_stride, act16, false, out_split != 0,
                                lo_off);
    if (a_wrap) set_a_wrap(p, a_wrap);
    gemm_launch(p, A_PLAIN, EPI_CONVT, ctx->dtype, ctx->stream, tile_cfg);
}

int32_t me_op_conv_transpose2x2_forms(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                      int32_t Cin, const void* w16, int32_t Cout, const float* bias,
                                      float* out32, void* out16, int32_t border16, int32_t act16,
                                      int32_t out_split, int32_t pixel_stride, int32_t lo_off, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    conv_transpose2x2_forms(ctx, in16, B, H, W, Cin, 0, w16, Cout, bias, out32, out16, border16, act16, out_split, pixel_stride, lo_off, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_conv_transpose2x2_forms_wrap(me_ctx* ctx, const void* in16, int32_t B, int32_t H, int32_t W,
                                           int32_t Cin, int32_t a_wrap, const void* w16, int32_t Cout, const float* bias,
                                           float* out32, void* out16, int32_t border16, int32_t act16,
                                           int32_t out_split, int32_t pixel_stride, int32_t lo_off, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    conv_transpose2x2_forms(ctx, in16, B, H, W, Cin, a_wrap, w16, Cout, bias, out32, out16, border16, act16, out_split, pixel_stride, lo_off,
                            tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_conv_transpose2x2_pair(me_ctx* ctx, int32_t B, int32_t H, int32_t W, int32_t Cout, const void* in16_a, int32_t Cin_a,
                                     const void* w16_a, const void* in16_b, int32_t Cin_b, int32_t a_wrap_b, const void* w16_b,
                                     const float* bias_b, float* out32, void* out16, int32_t border16, int32_t act16, int32_t grid_cap,
                                     int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(in16_a && w16_a && in16_b && w16_b && out32 && out16, ME_ERR_BAD_ARG, "me_op_conv_transpose2x2_pair: null pointer");
    admit_op_conv_transpose2x2_pair(B, H, W, Cout, Cin_a, Cin_b, a_wrap_b, act16, grid_cap);
    const GemmParams first = convt_params(in16_a, B, H, W, Cin_a, w16_a, Cout, nullptr, nullptr, out16, border16 != 0, 0, act16);
    GemmParams second = convt_params(in16_b, B, H, W, Cin_b, w16_b, Cout, bias_b, nullptr, nullptr, false, 0, ACT_NONE);
    if (a_wrap_b) set_a_wrap(second, a_wrap_b);
    GemmParams p = chain_convt(first, second, out32);
    p.grid_cap = grid_cap;
    gemm_launch(p, A_PLAIN, EPI_CONVT, ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

int32_t me_op_patch_embed(me_ctx* ctx, const void* patches16, int32_t windows, int32_t P, int32_t C, const void* W16,
                          const float* bias, const float* pos, float* tokens32, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(patches16 && W16 && bias && pos && tokens32, ME_ERR_BAD_ARG, "me_op_patch_embed: null pointer");
    admit_op_patch_embed(windows, P, C);
    gemm_launch(patch_embed_params(windows, P, C, patches16, W16, bias, pos, tokens32), A_PLAIN, EPI_PATCH_EMBED, ctx->dtype, ctx->stream,
                tile_cfg);
    ME_API_END(ctx)
}

// ---- the layout / element-wise kernels (elementwise.hip): the launch helpers trust the pipeline, so an entry checks its pointers
// here and its shapes in admission.h (admit_grid, admit_map, admit_op_*) ----
int32_t me_op_bilinear(me_ctx* ctx, const float* src32, void* dst16, int32_t planes, int32_t in_size, int32_t out_size,
                       int32_t align_corners) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src32 && dst16, ME_ERR_BAD_ARG, "me_op_bilinear: null pointer");
    admit_op_bilinear(planes, in_size, out_size);
    bilinear_launch(src32, dst16, planes, in_size, out_size, align_corners ? 1 : 0, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_patchify(me_ctx* ctx, const void* x0, const void* x1, const void* x2, void* patches, int32_t batch,
                       int32_t grid) {
    ME_API_BEGIN(ctx)
    ME_CHECK(x0 && x1 && x2 && patches, ME_ERR_BAD_ARG, "me_op_patchify: null pointer");
    admit_op_patchify(batch, grid);
    patchify_launch(x0, x1, x2, patches, batch, grid, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_patchify_windows(me_ctx* ctx, const void* xs16, void* patches, int32_t windows, int32_t grid) {
    ME_API_BEGIN(ctx)
    ME_CHECK(xs16 && patches, ME_ERR_BAD_ARG, "me_op_patchify_windows: null pointer");
    admit_op_patchify_windows(windows, grid);
    patchify_windows_launch(xs16, patches, windows, grid, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_cls_rows(me_ctx* ctx, float* tokens, const float* cls, const float* pos, int32_t windows, int32_t tpw,
                       int32_t dim) {
    ME_API_BEGIN(ctx)
    ME_CHECK(tokens && cls && pos, ME_ERR_BAD_ARG, "me_op_cls_rows: null pointer");
    admit_op_cls_rows(windows, tpw, dim);
    cls_rows_launch(tokens, cls, pos, windows, tpw, dim, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_merge(me_ctx* ctx, const float* src32, const void* src16, void* dst16, int32_t batch, int32_t wpi,
                    int32_t win0, int32_t steps, int32_t padding, int32_t grid, int32_t dim, int32_t split) {
    ME_API_BEGIN(ctx)
    ME_CHECK(dst16, ME_ERR_BAD_ARG, "me_op_merge: null pointer");
    admit_op_merge(batch, wpi, win0, steps, padding, grid, dim);
    merge_launch(src32, src16, dst16, batch, wpi, win0, steps, padding, grid, dim, ctx->dtype, ctx->stream, split ? 1 : 0);
    ME_API_END(ctx)
}

int32_t me_op_nchw32_to_nhwc(me_ctx* ctx, const float* src, float* dst32, void* dst16, int32_t batch, int32_t H,
                             int32_t W, int32_t C, int32_t border, int32_t relu16, int32_t split) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src && (dst32 || dst16) && (dst16 || (!border && !relu16 && !split)), ME_ERR_BAD_ARG, "me_op_nchw32_to_nhwc: null pointer");
    admit_map("me_op_nchw32_to_nhwc", batch, H, W, C);
    nchw32_to_nhwc_launch(src, dst32, dst16, batch, H, W, C, border ? 1 : 0, relu16 ? 1 : 0, ctx->dtype, ctx->stream, split ? 1 : 0);
    ME_API_END(ctx)
}

int32_t me_op_nhwc16_to_nchw32(me_ctx* ctx, const void* src16, float* dst, int32_t batch, int32_t H, int32_t W,
                               int32_t C, int32_t border, int32_t split) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src16 && dst, ME_ERR_BAD_ARG, "me_op_nhwc16_to_nchw32: null pointer");
    admit_map("me_op_nhwc16_to_nchw32", batch, H, W, C);
    nhwc16_to_nchw32_launch(src16, dst, batch, H, W, C, border ? 1 : 0, ctx->dtype, ctx->stream, split ? 1 : 0);
    ME_API_END(ctx)
}

int32_t me_op_nhwc32_to_nchw32(me_ctx* ctx, const float* src, float* dst, int32_t batch, int32_t H, int32_t W,
                               int32_t C) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src && dst, ME_ERR_BAD_ARG, "me_op_nhwc32_to_nchw32: null pointer");
    admit_map("me_op_nhwc32_to_nchw32", batch, H, W, C);
    nhwc32_to_nchw32_launch(src, dst, batch, H, W, C, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_nhwc32_to_16b(me_ctx* ctx, const float* src, void* dst16b, int32_t batch, int32_t H, int32_t W,
                            int32_t C, int32_t relu) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src && dst16b, ME_ERR_BAD_ARG, "me_op_nhwc32_to_16b: null pointer");
    admit_map("me_op_nhwc32_to_16b", batch, H, W, C);
    nhwc32_to_16b_launch(src, dst16b, batch, H, W, C, relu ? 1 : 0, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_concat_channels(me_ctx* ctx, const void* a16, const void* b16, void* dst16, int64_t pixels, int32_t Ca,
                              int32_t Cb) {
    ME_API_BEGIN(ctx)
    ME_CHECK(a16 && b16 && dst16, ME_ERR_BAD_ARG, "me_op_concat_channels: null pointer");
    admit_op_concat_channels(pixels, Ca, Cb);
    concat_channels_launch(a16, b16, dst16, pixels, Ca, Cb, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_fov_add(me_ctx* ctx, const float* lin, const float* low, void* dst16b, int32_t batch, int32_t grid,
                      int32_t C, int32_t tpw) {
    ME_API_BEGIN(ctx)
    ME_CHECK(lin && low && dst16b, ME_ERR_BAD_ARG, "me_op_fov_add: null pointer");
    admit_op_fov_add(batch, grid, C, tpw);
    fov_add_relu_launch(lin, low, dst16b, batch, grid, C, tpw, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_fov_final(me_ctx* ctx, const void* x16, const float* w, const float* bias, float* fov_deg, float* f_norm,
                        int32_t batch, int32_t k, int32_t C) {
    ME_API_BEGIN(ctx)
    ME_CHECK(x16 && w && bias && f_norm, ME_ERR_BAD_ARG, "me_op_fov_final: null pointer");
    admit_op_fov_final(batch, k, C);
    fov_final_launch(x16, w, bias, fov_deg, f_norm, batch, k, C, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_quantize_fp8(me_ctx* ctx, const void* src16, int64_t rows, int32_t K, int32_t weight_layout,
                           uint8_t* dst8, uint8_t* scales) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src16 && dst8 && scales, ME_ERR_BAD_ARG, "me_op_quantize_fp8: null pointer");
    quantize_f16_to_fp8_launch(src16, dst8, scales, rows, K, weight_layout, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_attention_fp8(me_ctx* ctx, const void* qkv16, uint8_t* out8, uint8_t* out8_scale, int32_t windows,
                            int32_t tokens, int32_t heads) {
    ME_API_BEGIN(ctx)
    ME_CHECK(qkv16 && out8 && out8_scale, ME_ERR_BAD_ARG, "me_op_attention_fp8: null pointer");
    attention_launch(qkv16, nullptr, windows, tokens, heads, ctx->dtype, ctx->stream, nullptr, out8, out8_scale,
                     cdiv((int64_t)windows * tokens, 128));
    ME_API_END(ctx)
}

int64_t me_op_scale_index(int64_t row, int32_t kblock, int64_t rows, int32_t weight_layout) {
    return weight_layout ? w_scale_index(row, kblock, rows / 64) : a_scale_index(row, kblock, cdiv(rows, 128));
}

int32_t me_op_layernorm_fp8(me_ctx* ctx, const float* x32, const float* weight, const float* bias, uint8_t* y8,
                            uint8_t* yscale, int64_t rows, int32_t dim, float eps) {
    ME_API_BEGIN(ctx)
    ME_CHECK(x32 && weight && bias && y8 && yscale, ME_ERR_BAD_ARG, "me_op_layernorm_fp8: null pointer");
    layernorm_fp8_launch(x32, weight, bias, y8, yscale, rows, dim, eps, ctx->stream);
    ME_API_END(ctx)
}

// the three forms of me_op_linear_fp8 and me_op_linear_fp8_segments: the residual update of x32, fc1 (GELU) as the next GEMM's
// fp8 operand, or a plain 16-bit output
static GemmParams linear_fp8_params(int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale, const uint8_t* W8,
                                    const uint8_t* w_scale, const float* bias, const float* gamma, void* out16, uint8_t* out8,
                                    uint8_t* out8_scale, float* x32) {
    GemmParams p = x32 ? resid_params(M, N, K, A8, W8, bias, gamma, x32)
                       : linear_params(M, N, K, A8, W8, bias, out8 ? nullptr : out16, nullptr, out8 ? ACT_GELU : ACT_NONE);
    set_fp8_operands(p, a_scale, w_scale);
    if (!x32 && out8) set_out8(p, out8, out8_scale);
    return p;
}

int32_t me_op_linear_fp8(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale,
                         const uint8_t* W8, const uint8_t* w_scale, const float* bias, void* out16, uint8_t* out8,
                         uint8_t* out8_scale, const float* gamma, float* x32) {
    ME_API_BEGIN(ctx)
    if (x32) ME_CHECK(gamma && bias, ME_ERR_BAD_ARG, "me_op_linear_fp8: the residual form takes bias and gamma");
    const GemmParams p = linear_fp8_params(M, N, K, A8, a_scale, W8, w_scale, bias, gamma, out16, out8, out8_scale, x32);
    gemm_fp8_launch(p, x32 ? EPI_RESID_SCALE : EPI_STORE, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_linear_fp8_segments(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale,
                                  int32_t seg1, int32_t seg2, const uint8_t* const W8[3], const uint8_t* const w_scale[3],
                                  const float* const bias[3], const float* const gamma[3], void* out16, uint8_t* out8,
                                  uint8_t* out8_scale, float* x32) {
    ME_API_BEGIN(ctx)
    ME_CHECK(A8 && a_scale && W8 && w_scale && bias, ME_ERR_BAD_ARG, "me_op_linear_fp8_segments: null pointer");
    if (x32) ME_CHECK(gamma, ME_ERR_BAD_ARG, "me_op_linear_fp8_segments: the residual form takes gamma");
    GemmParams p = linear_fp8_params(M, N, K, A8, a_scale, nullptr, nullptr, nullptr, nullptr, out16, out8, out8_scale, x32);
    set_segments(p, seg1, seg2, seg_weights(W8, w_scale, bias, x32 ? gamma : nullptr));
    gemm_fp8_launch(p, x32 ? EPI_RESID_SCALE : EPI_STORE, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_linear_fp8_residual_layernorm(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const uint8_t* A8, const uint8_t* a_scale,
                                            int32_t seg1, int32_t seg2, const uint8_t* const W8[3], const uint8_t* const w_scale[3],
                                            const float* const bias[3], const float* const gamma[3], const float* const ln_w[3],
                                            const float* const ln_b[3], float eps, float* x32, uint8_t* xn8, uint8_t* xn_scale) {
    ME_API_BEGIN(ctx)
    ME_CHECK(A8 && a_scale && W8 && w_scale && bias && gamma && ln_w && ln_b && x32 && xn8 && xn_scale, ME_ERR_BAD_ARG,
             "me_op_linear_fp8_residual_layernorm: null pointer");
    admit_segment_weights("me_op_linear_fp8_residual_layernorm", seg1, seg2, W8, w_scale, bias, gamma, ln_w, ln_b);
    GemmParams p = linear_fp8_params(M, N, K, A8, a_scale, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, x32);
    set_segments(p, seg1, seg2, seg_weights(W8, w_scale, bias, gamma));
    set_fused_layernorm(ctx, p, "op.ln.stats", "op.ln.count." + std::to_string(N), LnSet{ln_w[0], ln_b[0], ln_w[1], ln_b[1], ln_w[2], ln_b[2]},
                        eps, nullptr, xn8, xn_scale);
    gemm_fp8_launch(p, EPI_RESID_SCALE, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_linear_segments(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1, int32_t seg2,
                              const void* const W16[3], const float* const bias[3], const float* const gamma[3],
                              void* out16, float* x32, int32_t act, int32_t tile_cfg) {
    ME_API_BEGIN(ctx)
    ME_CHECK(A16 && W16 && bias && (out16 || x32), ME_ERR_BAD_ARG, "me_op_linear_segments: null pointer");
    admit_op_linear_segments(M, seg1, seg2, W16, gamma, x32 != nullptr);
    GemmParams p = x32 ? resid_params(M, N, K, A16, nullptr, nullptr, nullptr, x32)
                       : linear_params(M, N, K, A16, nullptr, nullptr, out16, nullptr, act);
    set_segments(p, seg1, seg2, seg_weights(W16, nullptr, bias, x32 ? gamma : nullptr));
    gemm_launch(p, A_PLAIN, x32 ? EPI_RESID_SCALE : EPI_STORE, ctx->dtype, ctx->stream, tile_cfg);
    ME_API_END(ctx)
}

// me_op_attention_segments and me_op_layernorm_segments: the row-segmented forms of the merged ViT launches (pipeline.hip
// MergedVit, gemm_params.h RowSegs).  The kernels trust the row map, so a layout that does not fit its buffers is refused (admission.h).
int32_t me_op_attention_segments(me_ctx* ctx, const void* qkv16, void* out16, uint8_t* out8, uint8_t* out8_scale, int32_t windows,
                                 int32_t tokens, int32_t heads, int32_t prescaled, int64_t rows_total, int64_t seg1, int64_t seg2,
                                 int32_t win0, int32_t win1) {
    ME_API_BEGIN(ctx)
    ME_CHECK(qkv16 && (out16 || out8), ME_ERR_BAD_ARG, "me_op_attention_segments: null pointer");
    ME_CHECK(!(out16 && out8), ME_ERR_BAD_ARG, "me_op_attention_segments: ONE of out16 and out8");
    ME_CHECK(!out8 || out8_scale, ME_ERR_BAD_ARG, "me_op_attention_segments: out8 without its scales");
    admit_op_attention_segments(out8, windows, tokens, heads, rows_total, seg1, seg2, win0, win1);
    RowSegs segs;
    segs.seg1 = seg1, segs.seg2 = seg2, segs.win0 = win0, segs.win1 = win1;
    attention_launch(qkv16, out16, windows, tokens, heads, ctx->dtype, ctx->stream, &segs, out8, out8_scale,
                     out8 ? cdiv(rows_total, 128) : 0, prescaled != 0);
    ME_API_END(ctx)
}

int32_t me_op_layernorm_segments(me_ctx* ctx, const float* x32, const float* const weight[3], const float* const bias[3],
                                 int64_t seg1, int64_t seg2, void* y16, float* y32, uint8_t* y8, uint8_t* yscale, int64_t rows,
                                 int32_t dim, float eps) {
    ME_API_BEGIN(ctx)
    ME_CHECK(x32 && weight && bias && (y16 || y32 || y8), ME_ERR_BAD_ARG, "me_op_layernorm_segments: null pointer");
    ME_CHECK(!(y8 && (y16 || y32)), ME_ERR_BAD_ARG, "me_op_layernorm_segments: ONE of y16 / y32 and y8");
    ME_CHECK(!y8 || yscale, ME_ERR_BAD_ARG, "me_op_layernorm_segments: y8 without its scales");
    admit_op_layernorm_segments(weight, bias, seg1, seg2, y8, rows, dim);
    const int nseg = row_segment_count(seg1, seg2);
    RowSegs segs;
    segs.seg1 = seg1, segs.seg2 = seg2;
    if (nseg > 1) segs.w1 = weight[1], segs.b1 = bias[1];
    if (nseg > 2) segs.w2 = weight[2], segs.b2 = bias[2];
    if (y8) layernorm_fp8_launch(x32, weight[0], bias[0], y8, yscale, rows, dim, eps, ctx->stream, &segs);
    else layernorm_launch(x32, weight[0], bias[0], y16, y32, rows, dim, eps, ctx->dtype, ctx->stream, &segs);
    ME_API_END(ctx)
}

namespace {
// xn8 != nullptr: the normalised rows as MX fp8 + activation-layout scales (ceil(M / 128) tiles) instead of 16-bit
void linear_residual_layernorm_impl(me_ctx* ctx, const char* who, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1,
                                    int32_t seg2, const void* const W16[3], const float* const bias[3], const float* const gamma[3],
                                    const float* const ln_w[3], const float* const ln_b[3], float eps, float* x32, void* xn16,
                                    uint8_t* xn8, uint8_t* xn_scale) {
    ME_CHECK(A16 && W16 && bias && gamma && ln_w && ln_b && x32 && (xn16 || (xn8 && xn_scale)), ME_ERR_BAD_ARG, "%s: null pointer", who);
    admit_op_linear_residual_layernorm(who, M, N, seg1, seg2, W16, bias, gamma, ln_w, ln_b);
    GemmParams p = resid_params(M, N, K, A16, nullptr, nullptr, nullptr, x32);
    set_segments(p, seg1, seg2, seg_weights(W16, nullptr, bias, gamma));
    // (an arrival counter advances by N / 256 per launch and must start a launch at a multiple of that: one per N)
    set_fused_layernorm(ctx, p, "op.ln.stats", "op.ln.count." + std::to_string(N), LnSet{ln_w[0], ln_b[0], ln_w[1], ln_b[1], ln_w[2], ln_b[2]},
                        eps, xn16, xn8, xn_scale);
    gemm_launch(p, A_PLAIN, EPI_RESID_SCALE, ctx->dtype, ctx->stream, CFG_PP352);
}
}  // namespace

int32_t me_op_linear_residual_layernorm(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1,
                                        int32_t seg2, const void* const W16[3], const float* const bias[3],
                                        const float* const gamma[3], const float* const ln_w[3], const float* const ln_b[3],
                                        float eps, float* x32, void* xn16) {
    ME_API_BEGIN(ctx)
    ME_CHECK(xn16, ME_ERR_BAD_ARG, "me_op_linear_residual_layernorm: null pointer");
    linear_residual_layernorm_impl(ctx, "me_op_linear_residual_layernorm", M, N, K, A16, seg1, seg2, W16, bias, gamma, ln_w, ln_b, eps,
                                   x32, xn16, nullptr, nullptr);
    ME_API_END(ctx)
}

int32_t me_op_linear_residual_layernorm_fp8(me_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A16, int32_t seg1,
                                            int32_t seg2, const void* const W16[3], const float* const bias[3],
                                            const float* const gamma[3], const float* const ln_w[3], const float* const ln_b[3],
                                            float eps, float* x32, uint8_t* xn8, uint8_t* xn_scale) {
    ME_API_BEGIN(ctx)
    ME_CHECK(xn8 && xn_scale, ME_ERR_BAD_ARG, "me_op_linear_residual_layernorm_fp8: null pointer");
    linear_residual_layernorm_impl(ctx, "me_op_linear_residual_layernorm_fp8", M, N, K, A16, seg1, seg2, W16, bias, gamma, ln_w, ln_b,
                                   eps, x32, nullptr, xn8, xn_scale);
    ME_API_END(ctx)
}

int32_t me_op_format_f64(me_ctx* ctx, const double* values, int64_t count, char* text, int32_t stride, int32_t* lengths) {
    ME_API_BEGIN(ctx)
    ME_CHECK(values && text && lengths && count >= 0, ME_ERR_BAD_ARG, "me_op_format_f64: bad argument");
    format_f64_launch(values, count, text, stride, lengths, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_ply_pack(me_ctx* ctx, const float* xyz, const uint8_t* vertex_rgb, int64_t nverts, const int32_t* faces,
                       int64_t nfaces, int64_t header_bytes, uint8_t* out) {
    ME_API_BEGIN(ctx)
    ME_CHECK(out && nverts >= 0 && nfaces >= 0 && header_bytes >= 0 && (xyz || nverts == 0) && (faces || nfaces == 0),
             ME_ERR_BAD_ARG, "me_op_ply_pack: bad argument");
    ME_CHECK(nverts <= (int64_t)INT32_MAX && nfaces <= (int64_t)1 << 40, ME_ERR_BAD_ARG, "me_op_ply_pack: %lld vertices, %lld faces",
             (long long)nverts, (long long)nfaces);
    const bool rgb = vertex_rgb && nverts > 0;
    const float* x = nverts ? (const float*)to_device(ctx, xyz, (size_t)nverts * 12, "op.ply.xyz") : nullptr;
    const uint8_t* c = rgb ? (const uint8_t*)to_device(ctx, vertex_rgb, (size_t)nverts * 3, "op.ply.rgb") : nullptr;
    const int32_t* f = nfaces ? (const int32_t*)to_device(ctx, faces, (size_t)nfaces * 12, "op.ply.faces") : nullptr;
    const int64_t body = ply_pack_bytes(nverts, rgb, nfaces, 0);
    if (body == 0) return ME_OK;
    // a host `out` is staged without its header: the first header_bytes of the caller's array are never written
    OutBuf o = out_buf(ctx, out + header_bytes, (size_t)body, "op.ply.out");
    ply_pack_launch(x, c, nverts, f, nfaces, o.staged ? 0 : header_bytes, o.staged ? (uint8_t*)o.dev : out, ctx->stream);
    finish(ctx, o);
    ME_API_END(ctx)
}

int32_t me_op_exclusive_scan_u32(me_ctx* ctx, const uint32_t* counts, int64_t n, uint64_t base, int32_t form, uint64_t* offsets) {
    ME_API_BEGIN(ctx)
    ME_CHECK(offsets && n >= 0 && (counts || n == 0), ME_ERR_BAD_ARG, "me_op_exclusive_scan_u32: bad argument");
    ME_CHECK(form == 0 || (form == 1 && n > 0), ME_ERR_BAD_ARG, "me_op_exclusive_scan_u32: form %d with %lld counts", form, (long long)n);
    const uint32_t* c = n ? (const uint32_t*)to_device(ctx, counts, (size_t)n * 4, "op.scan.counts") : nullptr;
    OutBuf o = out_buf(ctx, offsets, (size_t)(n + 1) * 8, "op.scan.out");
    if (form == 0) obj_offsets_launch(c, n, base, (uint64_t*)o.dev, ctx->stream);
    else jpeg_encode_scan_offsets(ctx, c, n, base, (uint64_t*)o.dev);
    finish(ctx, o);
    ME_API_END(ctx)
}

int32_t me_op_cast_to16(me_ctx* ctx, const float* src, void* dst16, int64_t count) {
    ME_API_BEGIN(ctx)
    cast_f32_to_16_launch(src, dst16, count, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_op_cast_to32(me_ctx* ctx, const void* src16, float* dst, int64_t count) {
    ME_API_BEGIN(ctx)
    cast_16_to_f32_launch(src16, dst, count, ctx->dtype, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_profile_enable(me_ctx* ctx, int32_t on) {
    ME_API_BEGIN(ctx)
    ME_HIP(hipStreamSynchronize(ctx->stream));
    Profiler& p = profiler();
    for (ProfEntry& e : p.entries) {
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
    }
    p.entries.clear();
    p.enabled = on != 0;
    ME_API_END(ctx)
}

int32_t me_profile_report(me_ctx* ctx, char* json, int64_t capacity) {
    ME_API_BEGIN(ctx)
    ME_CHECK(json && capacity > 2, ME_ERR_BAD_ARG, "me_profile_report: no buffer");
    ME_HIP(hipStreamSynchronize(ctx->stream));
    struct Agg {
        double ms = 0, flops = 0, bytes = 0;
        long count = 0;
    };
    std::map<std::string, Agg> agg;
    for (ProfEntry& e : profiler().entries) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.e0, e.e1) != hipSuccess) continue;
        Agg& a = agg[e.name];
        a.ms += ms, a.flops += e.flops, a.bytes += e.bytes, a.count += 1;
    }
    std::string out = "[";
    bool first = true;
    for (auto& kv : agg) {
        char line[512];
        snprintf(line, sizeof line,
                 "%s{\"kernel\": \"%s\", \"launches\": %ld, \"total_ms\": %.6f, \"flops\": %.6e, "
                 "\"bytes\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.count, kv.second.ms, kv.second.flops,
                 kv.second.bytes);
        out += line;
        first = false;
    }
    out += "]";
    ME_CHECK((int64_t)out.size() + 1 <= capacity, ME_ERR_BAD_ARG, "me_profile_report: buffer too small");
    memcpy(json, out.c_str(), out.size() + 1);
    ME_API_END(ctx)
}

int32_t me_op_gemm_config_count(void) { return gemm_num_configs(); }
const char* me_op_gemm_config_name(int32_t cfg) { return gemm_config_name(cfg); }

}  // extern "C"
