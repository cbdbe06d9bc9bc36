// Context, packed weights and stage functions of the Depth Pro forward pass.
#pragma once
#include <exception>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../host/image_io.hpp"
#include "common.h"

namespace me {

// How a checkpoint tensor (PyTorch layout) is packed into the device arena.
enum PackKind : int32_t {
    PK_VEC_F32 = 0,  // any shape -> flat f32 (biases, LayerNorm, LayerScale, cls/pos)
    PK_MAT_16 = 1,   // [N][K...] row-major -> 16-bit [N][K]  (Linear, 1x1 conv, patch embed)
    PK_CONV_16 = 2,  // Conv2d [Cout][Cin][kh][kw] -> 16-bit [Cout][kh*kw][Cin]
    PK_CONVT_16 = 3, // ConvTranspose2d [Cin][Cout][2][2] -> 16-bit [(dy*2+dx)*Cout + co][Cin]
    PK_CONVK_F32 = 4 // Conv2d [1][Cin][k][k] -> f32 [k][k][Cin]  (fov.head.4)
};

struct WeightSlot {
    std::string name;
    std::vector<int64_t> dims;
    PackKind kind;
    size_t offset = 0, bytes = 0;
    bool loaded = false;
    // the K axis is stored twice, [W | W] per row / per tap: the consumer reads a split [hi | lo] activation
    // operand of twice the depth (pipeline.hip, "split operands")
    bool dup = false;
    int64_t numel() const {
        int64_t n = 1;
        for (auto d : dims) n *= d;
        return n;
    }
};

struct VitBlockW {
    const float *ln1_w, *ln1_b, *qkv_b, *proj_b, *ls1, *ln2_w, *ln2_b, *fc1_b, *fc2_b, *ls2;
    const void *qkv_w, *proj_w, *fc1_w, *fc2_w;
    // ME_DTYPE_FP8: MX fp8 copies of the four linears (e4m3 bytes [N][K] + e8m0 block scales in the weight
    // layout of mx_fp8.h), quantised on the device from the 16-bit arena when the weights are finalized
    const uint8_t *qkv_w8 = nullptr, *qkv_ws = nullptr, *fc1_w8 = nullptr, *fc1_ws = nullptr, *fc2_w8 = nullptr,
                  *fc2_ws = nullptr, *proj_w8 = nullptr, *proj_ws = nullptr;
};
struct VitW {
    const void* patch_w;
    const float *patch_b, *cls, *pos, *norm_w, *norm_b;
    std::vector<VitBlockW> blocks;
};
struct UpsampleW {
    const void* conv;               // 1x1 [dim_int][C]
    std::vector<const void*> convt; // packed [4*Cout][Cin]
    std::vector<int> cin, cout;
    int dim_int;
};
struct RcuW {
    const void* w[2];
    const float* b[2];
};
struct FusionW {
    RcuW resnet1, resnet2;
    const void* deconv;  // null at level 0
    const void* out_w;
    const float* out_b;
    // SPLIT_FUSION_OUT, levels 1-4: out_conv o deconv composed into ONE ConvTranspose (both are linear and
    // nothing sits between them, decoder.rs:95-101), packed [(dy,dx,co)][W_hi | W_hi | W_lo] against [hi | lo | hi]
    // activations; null when the two run as separate launches
    const void* fused_w = nullptr;
};
struct ModelW {
    VitW vit[3];
    UpsampleW up_latent0, up_latent1, up0, up1, up2;
    const void* up_lowres_w;
    const float* up_lowres_b;
    const void* fuse_w;
    const float* fuse_b;
    const void* dec_convs[5];  // [i] for level i (null for level 0)
    FusionW fusions[5];
    const void *head0_w, *head1_w, *head2_w;
    // derived (weights.hip compose_head): head.1 (ConvTranspose 2x2 s2) and head.2 (conv 3x3) as ONE 3x3 convolution on the
    // half-resolution map with 4 x 32 output channels (output phase (dy, dx) x channel), [128][9][Cmid] 16-bit; head_fused_b:
    // f32 [32] bias of interior pixels, then [9][32] the share of each 3x3 tap in it (taken out again where the tap falls
    // outside the full-resolution image), then [32] head.4.weight padded with zeros beyond head_dims[0].  Null when the composition does not apply (SPLIT_HEAD).
    const void* head_fused_w = nullptr;
    const float* head_fused_b = nullptr;
    // derived (weights.hip compose_features): fusions[0].out_conv and head.0 as ONE 3x3 convolution of out_conv's input,
    // [dec / 2][9][dec] 16-bit; feat_fused_b: f32 [dec / 2] bias + [9][dec / 2] per-tap shares
    const void* feat_fused_w = nullptr;
    const float* feat_fused_b = nullptr;
    const float *head0_b, *head1_b, *head2_b, *head4_w, *head4_b;
    const void *fov_lin_w, *fov_down_w, *fov_h0_w, *fov_h2_w;
    const float *fov_lin_b, *fov_down_b, *fov_h0_b, *fov_h2_b, *fov_h4_w, *fov_h4_b;
};

// Split operands.  Every 16-bit MFMA operand costs one rounding of 2^-11 relative; on the un-diluted chain
// tokens -> upsample convs -> ... -> fusion out_conv -> head (no residual path beside it) those roundings are
// most of the depth error against the fp32 reference.  A stage listed here stores its 16-bit outputs as
// hi = T(v), lo = T(v - hi) in twice the channels, and its consumer runs the same kernel over K' = 2K against
// [W | W]: the product sees v to ~2^-22 at twice the MFMA work of that (small) layer.
enum SplitStage : int32_t {
    SPLIT_UPSAMPLE = 1,  // encoder.rs:307-325 upsample_* / upsample_lowres / fuse_lowres (A operands from merge)
    SPLIT_FUSION_OUT = 2,  // decoder.rs:95-101 deconv + out_conv of every fusion block
    SPLIT_HEAD = 4,        // mod.rs:323-333 head convs
    SPLIT_DEC_CONVS = 8    // decoder.rs:189-195 convs[i-1] on the encodings
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// One axis of the Lanczos3 resampler (resample.hip): the host-built table of lanczos_table.cpp on the device.
// span[o] = {left, count}; the i-th weight of output index o is w[i * len_out + o] (tap-major, so that neighbouring
// lanes of the horizontal pass read neighbouring words).
struct ResampleTable {
    int32_t len_in = 0, len_out = 0;
    int32_t run = 0;          // output pixels per workgroup of the horizontal pass; 0: its span does not fit the LDS
    int32_t lds_floats = 0;   // floats of LDS that run needs
    int2* span = nullptr;
    float* w = nullptr;
    uint64_t stamp = 0;       // last use, for eviction
};

struct WeightPackState;  // weight_pack_state.h: the device packer's staging ring, the last load's report

// A pinned host staging buffer that one asynchronous upload at a time reads (the photo decoders, input_api.hip): grown to
// the high-water mark; `uploaded` is recorded behind every upload, and the next call waits for it on the host before it
// writes or frees the buffer (calls may be queued without a synchronise between them).
struct PinnedUpload {
    void* host = nullptr;
    size_t capacity = 0;
    hipEvent_t uploaded = nullptr;
    bool pending = false;
    void* reserve(size_t bytes) {
        if (!uploaded) ME_HIP(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        if (pending) {
            ME_HIP(hipEventSynchronize(uploaded));
            pending = false;
        }
        if (bytes > capacity) {
            if (host) ME_HIP(hipHostFree(host));
            host = nullptr, capacity = 0;
            ME_HIP(hipHostMalloc(&host, bytes, hipHostMallocDefault));
            capacity = bytes;
        }
        return host;
    }
    void uploaded_on(hipStream_t stream) {
        ME_HIP(hipEventRecord(uploaded, stream));
        pending = true;
    }
    void release() {
        if (host) (void)hipHostFree(host);
        if (uploaded) (void)hipEventDestroy(uploaded);
        *this = PinnedUpload();
    }
};

// The timing marks around the legs of a context's last call of one kind: events made on first use, kept for the next call.
struct LegMarks {
    std::vector<hipEvent_t> ev;
    hipEvent_t at(size_t i) {
        while (ev.size() <= i) {
            hipEvent_t e = nullptr;
            ME_HIP(hipEventCreate(&e));
            ev.push_back(e);
        }
        return ev[i];
    }
    void record(size_t i, hipStream_t stream) { ME_HIP(hipEventRecord(at(i), stream)); }
    double ms(size_t a, size_t b) {
        float t = 0.f;
        ME_HIP(hipEventElapsedTime(&t, at(a), at(b)));
        return (double)t;
    }
    void destroy() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
    }
};

}  // namespace me

// The opaque C handle.
// me_last_jpeg_entropy: the last attempt at decoding a JPEG scan on the device (jpeg_entropy.hip)
struct JpegEntropyReport {
    int64_t where = 0;          // 0: the host decoder made the coefficients, 1: the device
    int64_t reason = 0;         // matrix_eyes::JpegEntropyDecline when where == 0 after an attempt
    int64_t segments = 0, subseqs = 0, subseq_bits = 0;
    int64_t rounds = 0;         // sync rounds, the confirming one included
    int64_t upload_bytes = 0;
    int64_t workgroups = 0;     // of each entropy kernel
    double ms[3] = {0, 0, 0};   // host marker scan and destuffing (wall clock), upload, entropy kernels (HIP events)
};

// me_last_jpeg_encode: the context's last JPEG encode (jpeg_encode.hip)
struct JpegEncodeReport {
    int64_t blocks = 0;              // of the scan, dummy blocks included
    int64_t scan_bits = 0;           // before the padding
    int64_t stuffed = 0;             // 00 bytes inserted
    int64_t file_bytes = 0;
    int64_t fdct_groups = 0, wave_groups = 0, block_scan_groups = 0, stuff_groups = 0;   // workgroups per kernel
    int64_t capacity = 0;            // bytes of the file buffer the encode was sized for
    bool downloaded = false;         // the file was copied to the host (the sixth leg)
};

struct me_ctx {
    int device = 0;
    int32_t dtype = ME_DTYPE_F16;
    // ME_DTYPE_FP8 (BASELINE configs[3]): `dtype` is ME_DTYPE_F16 for every 16-bit operand, and the qkv / fc1 /
    // fc2 linears of the three ViTs run on MX block-scaled fp8 (gemm_fp8.hip)
    bool fp8 = false;
    // which linears of a block run on fp8 in an ME_DTYPE_FP8 context: 1 = qkv, 2 = proj, 4 = fc1, 8 = fc2
    // (me_model_config.fp8_linears; 0 there means all four)
    int32_t fp8_mask = 0;
    char* arena8 = nullptr;  // the fp8 weight copies (derived data: rebuilt after finalize / adopt / broadcast)
    size_t arena8_bytes = 0;
    // Stages whose 16-bit activation operands are carried as hi + lo pairs (me::SplitStage bits)
    int32_t split_mask = 0;
    bool split(int stage_bit) const { return (split_mask & stage_bit) != 0; }
    me_model_config cfg;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // The side branch of extract_depth (api.hip extract_depth_impl): the latency-bound low-resolution decoder levels and
    // the FOV tail run on `side_stream` beside the bandwidth-bound ConvTranspose chains of the encoder's two latents,
    // forked and joined by events (captured into the step's hipGraph like any other dependency).  Opt-in (ME_OVERLAP_TAIL=1); a
    // progress callback or per-kernel timing keep the step on one stream.
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap_tail = true;
    // persistent GEMM launches issued while the side branch is in flight leave this many of the 256 CUs to it
    // (GemmParams::grid_cap); 0: no cap
    int32_t grid_cap = 0;
    std::string last_error;
    me_progress_fn progress = nullptr;
    void* progress_user = nullptr;
    // SplitProgressListener (mod.rs:374-414): a stage's positions in [0,1] are mapped into this range
    float prog_lo = 0.0f, prog_hi = 1.0f;

    // weights
    std::vector<me::WeightSlot> slots;
    std::map<std::string, int> slot_by_name;
    char* arena = nullptr;
    size_t arena_bytes = 0;
    bool finalized = false;
    me::ModelW w;
    std::vector<std::string> unused_weights;  // checkpoint keys me_load_checkpoint_pt skipped
    // derived weights (composed deconv + out_conv per fusion level): arena offsets, and the host copies of their
    // two factors kept from me_load_weight until me_weights_finalize composes them
    size_t fused_off[5] = {0, 0, 0, 0, 0};
    size_t head_fused_off = 0;   // 0: not composed
    size_t feat_fused_off = 0;   // 0: not composed
    bool features_pre = false;   // "features.16b" holds out_conv's INPUT (stage_decoder_levels with the composed head[0])
    // Decoder level 0 takes x0 + x1 from ONE chained ConvTranspose launch (pipeline.hip enc0_sum_applies): set by
    // extract_depth for the length of a call, never by the stage-wise entries.  The latent0 chain then stops before its last
    // ConvTranspose and leaves that launch's operand (enc0_last_in, a side x side map), level 1 does not launch its composed one.
    bool enc0_sum = false;
    const void* enc0_last_in = nullptr;
    int enc0_last_side = 0;
    std::map<std::string, std::vector<float>> factor_keep;
    // me_ctx_set_weight_packer: 0 the host packer (load_weight's loops on one core, a synchronous upload per tensor),
    // 1 the device packer (weight_pack.hip: raw bytes through a pinned ring, one pack kernel per tensor on the stream)
    int32_t weight_packer = 0;
    me::WeightPackState* wp = nullptr;

    // me_status_flags: one device word the kernels OR bits into (ME_STATUS_OVERFLOW_16BIT: an f16 operand store
    // met a magnitude beyond 65504, common.h raise_overflow16)
    unsigned* status_dev = nullptr;
    // Pinned host mirror of the status word: every step whose result stays on the device ends with an asynchronous copy
    // of the word into it, so the NEXT entry into the library sees what earlier asynchronous steps raised without
    // synchronising anything (api.hip check_pending_status).
    volatile unsigned* status_host = nullptr;
    // The fused residual + LayerNorm launch waits on sibling workgroups inside the launch (gemm_core.h
    // resid_ln_epilogue), which needs them co-resident.  When a step reports ME_STATUS_SYNC_TIMEOUT (a second tenant on
    // the device, a CU mask the runtime does not report) the context latches this, the step is run again with the
    // stand-alone LayerNorm launches (bit for bit the ME_LN_FUSE=0 result), and fusion stays off for the context.
    bool ln_fuse_off = false;
    int32_t ln_fallbacks = 0;     // steps re-run because of it (me_ln_fusion_state)
    std::string ln_fuse_note;     // logged once: why fusion went off

    // Write-behind of mesh files (me_ctx_set_write_behind; file_write.hip): the bytes of mesh call i are written to their
    // file by a host thread while the caller goes on to image i + 1.  One slot = a pinned host staging buffer (the file's D2H
    // copy, mesh_writer.hip) + the write that reads it; slot 0 alone serves the synchronous form.  Slots are used in
    // turn, so at most `write_behind` writes are in flight.  A failed write is reported by the call that next waits
    // for it (a later me_output_mesh reusing the slot, or me_output_flush).
    int write_behind = 0;  // 0: synchronous; n >= 2: files in flight
    struct WriteSlot {
        void* pinned = nullptr;
        size_t pinned_bytes = 0;
        std::thread th;
        bool active = false;
        int32_t code = 0;
        std::string msg;
        std::string dest;  // the file the pending write goes to
    };
    std::vector<WriteSlot> write_slots = std::vector<WriteSlot>(1);
    int write_next = 0;
    // legs of the last me_output_mesh call that made its file on the device (.obj, .ply or .glb), host wall clock: [0] mesh
    // indexing + vertex kernels, [1] the kernels that format the text or pack the records, [2] D2H copy of the file,
    // [3] file write, or handing it to the write-behind thread (me_last_mesh_timing)
    double mesh_ms[4] = {0, 0, 0, 0};
    int64_t mesh_bytes = 0;

    // Output overlap (me_ctx_set_output_overlap; BASELINE configs[4]: depth -> stereogram -> mesh per image, many images):
    // the output back end's kernels, copies and their host waits run on `out_stream`, ordered behind the extract_depth step
    // that PRODUCED the depth buffer they read -- not behind whatever the caller has queued on the main stream since -- so
    // image i + 1's depth step runs on the GPU while the host waits for image i's mesh counts, text and D2H copy.  A depth
    // buffer is known by its address range: the step that writes it records `produced` behind itself, every output call
    // on a buffer leaves `consumed` behind itself, and the next step that writes the range waits for that (the caller
    // alternates two buffers).  api.hip OutputScope.
    bool output_overlap = false;
    hipStream_t out_stream = nullptr;
    struct DepthSlot {
        const char* base = nullptr;
        size_t bytes = 0;
        hipEvent_t produced = nullptr, consumed = nullptr;
        bool has_produced = false, has_consumed = false;
        uint64_t stamp = 0;
    };
    DepthSlot depth_slots[4];
    uint64_t depth_stamp = 0;

    // persistent workspaces keyed by site name (no aliasing: zero borders stay zero)
    std::map<std::string, me::DevBuf> bufs;

    // Lanczos3 tables by (len_in, len_out), at most kMaxResampleTables; one is only freed behind a synchronise of
    // both streams (resample.hip resample_table): a queued kernel may still read it
    static constexpr size_t kMaxResampleTables = 16;
    std::vector<me::ResampleTable> rs_tables;
    uint64_t rs_stamp = 0;

    // The whole extract_depth step as one hipGraph (shapes are static per batch size).  A call whose pointers
    // all live on the device and that needs no host callback is enqueued eagerly the first time it is seen,
    // captured the second time and replayed with one hipGraphLaunch from then on; anything that changes what the
    // captured launches would do (weights, stream, another batch or another pointer) drops the graph.
    struct GraphKey {
        const void* in = nullptr;
        const void* f_norm = nullptr;
        void* depth = nullptr;
        void* fov = nullptr;
        hipStream_t stream = nullptr;
        int32_t batch = 0, entry = 0;
        uint64_t weights_generation = 0;
        bool operator==(const GraphKey& o) const {
            return in == o.in && f_norm == o.f_norm && depth == o.depth && fov == o.fov && stream == o.stream &&
                   batch == o.batch && entry == o.entry && weights_generation == o.weights_generation;
        }
    };
    bool graph_enabled = false;   // me_ctx_set_graph / ME_GRAPH=1: measured equal (f16) to 1 % slower (fp8) than eager
    bool capturing = false;       // site_buf must not allocate while a capture is open
    bool graph_seen = false, graph_refused = false;
    GraphKey graph_key;           // of graph_exec, or of the eager call last seen
    hipGraphExec_t graph_exec = nullptr;
    uint64_t weights_generation = 0;
    int64_t graph_launches = 0;   // replays so far (me_graph_launch_count)
    void drop_graph() {
        if (graph_exec) {
            // replays are asynchronous: a launch still queued on the stream references the exec's kernarg / node
            // memory, so the stream is drained before the exec goes
            (void)hipStreamSynchronize(stream);
            (void)hipGraphExecDestroy(graph_exec);
        }
        graph_exec = nullptr, graph_seen = false, graph_refused = false;
    }
    // Layout of the weight arena as a hash (FNV-1a over dtype, geometry, split mask and every slot's offset / size):
    // ranks that exchange arenas (me_bcast_weights, me_weights_adopt) must agree on it
    uint64_t arena_layout_hash() const {
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](uint64_t v) {
            for (int i = 0; i < 8; ++i) h = (h ^ ((v >> (8 * i)) & 0xff)) * 1099511628211ull;
        };
        mix((uint64_t)dtype), mix(fp8 ? 1 : 0), mix((uint64_t)split_mask), mix(arena_bytes);
        for (const me::WeightSlot& s : slots) mix(s.offset), mix(s.bytes), mix((uint64_t)s.kind), mix(s.dup ? 1 : 0);
        for (int i = 0; i < 5; ++i) mix(fused_off[i]);
        mix(head_fused_off);
        mix(feat_fused_off);
        return h;
    }

    // Photo input (input_api.hip; DESIGN.md "The photo front end").  Kept behind everything the model's units read, so
    // that a change here moves no offset they use.  One staging buffer and one set of marks per format: a JPEG and a PNG
    // decode queued back to back never share a buffer, and each format's timing report outlives the other's decodes.
    // JPEG decoding (jpeg_decode.hip): jpeg_upload is what the entropy decoder fills and the upload reads; jpeg_marks are
    // the marks around the legs of the last decode (me_last_jpeg_timing).
    me::PinnedUpload jpeg_upload;
    me::LegMarks jpeg_marks;
    bool jpeg_timed = false, jpeg_timed_download = false;
    double jpeg_entropy_ms = 0.0;
    // The entropy leg on the device (jpeg_entropy.hip; me_ctx_set_jpeg_entropy): 0 host, 1 device.  The report of the last
    // attempt (me_last_jpeg_entropy), the marks around its upload and kernels, and the pinned words its status comes back in.
    int32_t jpeg_entropy_mode = 0;
    JpegEntropyReport jpeg_entropy_report;
    bool jpeg_entropy_reported = false;
    me::LegMarks jpeg_entropy_marks;
    int32_t* jpeg_entropy_status = nullptr;
    // JPEG encoding (jpeg_encode.hip): the report of the last encode and the marks around its legs (me_last_jpeg_encode)
    JpegEncodeReport jpeg_encode_report;
    bool jpeg_encode_reported = false;
    me::LegMarks jpeg_encode_marks;
    // PNG decoding (png_decode.hip): png_upload is what zlib inflates into and the uploads read; png_status: the pinned word
    // the finish kernel's palette status comes back in.  png_marks: the marks of the last decode (me_last_png_timing): three
    // per band (before its upload, between upload and unfilter launch, behind the launch), then before and behind the finish
    // kernel and behind the download.
    me::PinnedUpload png_upload;
    int32_t* png_status = nullptr;
    me::LegMarks png_marks;
    int32_t png_timed_bands = 0;
    bool png_timed = false, png_timed_download = false;
    double png_inflate_ms = 0.0;
    // The keyed stereogram noise (stereogram_noise.hip; me_last_stereogram_noise), behind the photo fields for the same
    // reason: who asked for the last fill (0 nobody yet, 1 me_stereogram_noise, 2 a keyed stereogram entry), the words it
    // generated and the marks around the kernel
    int32_t stereo_noise_path = 0;
    int64_t stereo_noise_words = 0;
    me::LegMarks stereo_noise_marks;
    // steps enqueued (eagerly or into a capture) with the side branch forked (me_side_branch_count); a replay enqueues nothing
    int64_t side_branch_steps = 0;

    // geometry helpers
    int g() const { return cfg.grid; }
    int P() const { return cfg.grid * cfg.grid; }
    int T() const { return cfg.grid * cfg.grid + 1; }
    int S() const { return 64 * cfg.grid; }
    int C() const { return cfg.embed_dim; }
};

namespace me {

void build_weight_table(me_ctx* ctx);
void resolve_weights(me_ctx* ctx);
void load_weight(me_ctx* ctx, const char* name, const void* data, int32_t weight_dtype,
                 const int64_t* dims, int32_t ndim);
void finalize_weights(me_ctx* ctx);
void load_checkpoint_pt(me_ctx* ctx, const char* path);
// (re)derives the MX fp8 weight copies from the 16-bit arena (fp8 contexts; no-op otherwise)
void build_fp8_weights(me_ctx* ctx);
// what me_weights_adopt does: an arena that arrived from elsewhere (a broadcast, a caller's collective, the cache file)
void adopt_weights(me_ctx* ctx);
// weight_pack.hip: the device packer behind load_weight (the slot's tensor, raw, from a host or device pointer: staged,
// uploaded and packed asynchronously on the context's stream), the wait finalize_weights starts with, and the arena cache
void device_pack_weight(me_ctx* ctx, WeightSlot& s, const void* data, int32_t weight_dtype);
void weight_pack_sync(me_ctx* ctx);
void free_weight_pack(me_ctx* ctx);

// thrown by site_buf when a buffer would have to be (re)allocated while a stream capture is open
struct CaptureAbort {};
// persistent device buffer for a pipeline site; zero-filled when (re)allocated
void* site_buf(me_ctx* ctx, const std::string& name, size_t bytes);
// gemm_params.h set_fused_layernorm with the two scratch buffers taken from the context (count_site: one per N, the counter's stride)
inline void set_fused_layernorm(me_ctx* ctx, GemmParams& p, const std::string& stats_site, const std::string& count_site,
                                const LnSet& ln, float eps, void* xn16, uint8_t* xn8, uint8_t* xn_scale) {
    const LnScratchBytes bytes = ln_scratch_bytes(p);
    void* stats = site_buf(ctx, stats_site, (size_t)bytes.stats);
    void* count = site_buf(ctx, count_site, (size_t)bytes.count);
    set_fused_layernorm(p, ln, eps, xn16, xn8, xn_scale, (unsigned long long*)stats, (unsigned*)count);
}

// host-or-device pointer helpers
bool is_device_ptr(const void* p);
// returns a device pointer holding `bytes` of `p` (copying through site buffer `name` if host)
const void* to_device(me_ctx* ctx, const void* p, size_t bytes, const std::string& name);
// device result -> caller pointer (host or device)
void from_device(me_ctx* ctx, void* dst, const void* src_dev, size_t bytes);
// a caller's output pointer (api.hip): itself if it is device memory, else site buffer `name`, which finish copies out
struct OutBuf {
    void* dev = nullptr;
    void* user = nullptr;
    size_t bytes = 0;
    bool staged = false;
};
OutBuf out_buf(me_ctx* ctx, void* user, size_t bytes, const std::string& name);
void finish(me_ctx* ctx, const OutBuf& o);
// api.hip: the calling thread's error text of the entries that take no context (me_last_error(nullptr))
std::string& create_error();

// ---- stages (all device pointers; see pipeline.hip) ----
struct VitTaps {
    // called after block `index` with the f32 token stream [W*T][C]
    void (*fn)(void* user, int index, const float* tokens) = nullptr;
    void* user = nullptr;
};
// patches16 [W*P][768] -> tokens32 (residual stream, scratch) ; final LayerNorm written to
// final16 (16-bit) and/or final32.  `tag` names the scratch buffers (one set per stream).
void vit_forward(me_ctx* ctx, int which, const void* patches16, int W, const VitTaps& taps,
                 void* final16, float* final32, const std::string& tag, hipStream_t stream);

// with_fov: the FOV encoder (fov.rs:57-63 ViT + Linear) runs as a third row segment of the encoder's ViT
// launches; stage_fov_tail finishes it
void stage_encoder(me_ctx* ctx, const float* img32, int B, bool with_fov);
// the two halves of stage_encoder: everything up to encodings 2 - 4 (and the FOV encoder's Linear), then the two
// latent upsample chains (encodings 0 and 1, encoder.rs:307-309)
void stage_encoder_trunk(me_ctx* ctx, const float* img32, int B, bool with_fov);
void stage_encoder_latents(me_ctx* ctx, int B);
void stage_decoder(me_ctx* ctx, int B, bool want_features32);
// whether a whole extract_depth call of this batch may sum decoder level 0's two ConvTransposes in one launch (me_ctx::enc0_sum)
bool enc0_sum_applies(const me_ctx* ctx, int B);
// decoder levels `first` down to `last` (4 = lowest resolution ... 0); stage_decoder = levels 4 to 0
void stage_decoder_levels(me_ctx* ctx, int B, bool want_features32, int first, int last);
void stage_fov_vit(me_ctx* ctx, int B, hipStream_t s);
void stage_fov_tail(me_ctx* ctx, int B, float* fov_deg_dev);
// f_norm_dev [B]; clamp 0 = canonical (no clamp, f_norm ignored -> 1)
void stage_head(me_ctx* ctx, int B, const float* f_norm_dev, bool clamp, float* depth_dev, bool pre_image = false);

void report(me_ctx* ctx, float pos, const char* msg);

// Scope of one output back-end entry point (api.hip): with output overlap on, the context's stream is the output stream
// for the duration of the call, behind the step that produced `depth`; on exit the buffer's `consumed` event is left.
struct OutputScope {
    me_ctx* ctx;
    hipStream_t saved = nullptr;
    int slot = -1;
    bool active = false;
    OutputScope(me_ctx* c, const void* depth);
    ~OutputScope();
    OutputScope(const OutputScope&) = delete;
    OutputScope& operator=(const OutputScope&) = delete;
};

// resample.hip: DynamicImage::resize_exact(nw, nh, Lanczos3) for 8-bit RGB, device pointers, on ctx->stream
void resize_lanczos3_rgb8(me_ctx* ctx, const uint8_t* src_dev, int32_t w, int32_t h, uint8_t* dst_dev, int32_t nw, int32_t nh);
void free_resample_tables(me_ctx* ctx);
// api.hip: the sizes a resize entry accepts (ME_ERR_BAD_SHAPE otherwise, in the name of entry `who`)
void check_resize_shape(const char* who, int32_t w, int32_t h, int32_t nw, int32_t nh);

// jpeg_decode.hip: a JPEG file in host memory -> its oriented RGB picture [oh][ow][3] in device memory, on ctx->stream.
// Throws me::Error (ME_ERR_BAD_ARG with the host decoder's message for a file it refuses, ME_ERR_BAD_SHAPE for a size that
// does not match).  dst_dev == nullptr: into the context's own "jpeg.rgb" buffer; returns where the picture is.  want_w /
// want_h <= 0: any size; *ow / *oh receive the oriented size.
uint8_t* jpeg_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst_dev,
                          int32_t want_w, int32_t want_h, int32_t* ow, int32_t* oh);
void free_jpeg_scratch(me_ctx* ctx);
// the context's pinned staging buffer of `count` int16_t, once the upload of the call before has left it
inline int16_t* jpeg_pinned_buffer(me_ctx* ctx, size_t count) { return (int16_t*)ctx->jpeg_upload.reserve(count * sizeof(int16_t)); }
// The size first: a w x h picture under `orientation` is *ow x *oh, and a destination of another size (want_w / want_h > 0)
// is refused before any decoding.  `format`: "JPEG" / "PNG".
inline void oriented_size_or_refuse(const char* format, int32_t w, int32_t h, int32_t orientation, int32_t want_w, int32_t want_h,
                                    int32_t* ow, int32_t* oh) {
    const bool swap = orientation >= 5;
    *ow = swap ? h : w, *oh = swap ? w : h;
    ME_CHECK((want_w <= 0 && want_h <= 0) || (want_w == *ow && want_h == *oh), ME_ERR_BAD_SHAPE,
             "%s decode: the picture is %dx%d (orientation %d), the destination %dx%d", format, *ow, *oh, orientation, want_w, want_h);
}
// jpeg_entropy.hip: the scan's coefficients made on the device, into the "jpeg.coef" buffer.  subseq_bits 0: the default.
// False: declined (ctx->jpeg_entropy_report.reason), the host decoder is to run.
bool jpeg_entropy_decode(me_ctx* ctx, const std::vector<uint8_t>& file, int32_t subseq_bits,
                         matrix_eyes::JpegEntropyPlan& plan);
void free_jpeg_entropy_scratch(me_ctx* ctx);
// png_decode.hip: a PNG file in host memory -> its oriented RGB picture [oh][ow][3] in device memory, on ctx->stream;
// arguments, result and errors as jpeg_decode_rgb8 ("png.rgb" is the context's own buffer).  The host inflates into pinned
// memory and every finished band of rows is uploaded and unfiltered behind it.
uint8_t* png_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst_dev,
                         int32_t want_w, int32_t want_h, int32_t* ow, int32_t* oh);
// the unfilter leg alone: a filtered stream -> the reconstructed stream (same layout), device pointers, src == dst allowed;
// band_rows 0: the default
void png_unfilter(me_ctx* ctx, const uint8_t* src_dev, uint8_t* dst_dev, int32_t width, int32_t height, int32_t depth,
                  int32_t ctype, int32_t interlace, int32_t band_rows);
void free_png_scratch(me_ctx* ctx);
// png_encode.hip, jpeg_encode.hip: a finished file in the context's scratch, and the encoders that leave one there.  Both
// synchronise (the file's size comes back to the host); the entries (output_api.hip) check the arguments first.
struct DeviceFile {
    const uint8_t* dev = nullptr;
    int64_t bytes = 0;
};
void check_png_shape(const char* who, int32_t w, int32_t h);
DeviceFile png_encode_device(me_ctx* ctx, const uint8_t* rgb_dev, int32_t w, int32_t h);
void check_jpeg_encode_args(const char* who, int32_t w, int32_t h, int32_t quality, int32_t subsampling);
DeviceFile jpeg_encode_device(me_ctx* ctx, const uint8_t* rgb_any, int32_t w, int32_t h, int32_t quality, int32_t subsampling);
void free_jpeg_encode_scratch(me_ctx* ctx);
// stereogram_noise.hip: the keyed noise (chacha.h) on ctx->stream, device pointers.  The fill writes [out_h][out_w][3]
// (path: what me_last_stereogram_noise reports, 1 the noise entry, 2 a keyed entry); the keyed launch is stereogram_launch
// (its checks first) with the 32-byte key in place of the noise buffer: the fill into the context's "out.noise", then that.
void stereogram_noise_fill_launch(me_ctx* ctx, const uint8_t key[32], int32_t out_w, int32_t out_h, uint8_t* out_dev,
                                  int32_t path);
void stereogram_keyed_launch(me_ctx* ctx, const float* depth_dev, int32_t rows, int32_t cols, float min_depth, float max_depth,
                             const float* range_dev, int32_t out_w, int32_t out_h, float amplitude, const uint8_t key[32],
                             uint8_t* out_dev);
void free_stereogram_noise_scratch(me_ctx* ctx);

// file_write.hip: files written from host memory.
// A file serialised on the host: `head`, then each section's items in order; item(args, i, out) appends item i.  With
// `threads`, chunks of 32 Ki items are serialised by up to 12 threads and written with pwrite (the sequential loop's bytes).
typedef void (*AppendItem)(const void* args, int64_t i, std::string& out);
struct FileSection {
    int64_t count;
    AppendItem item;
    const void* args;
    bool threads;
};
void write_sections(const std::string& path, const std::string& head, const FileSection* sections, int count);
// a finished buffer into a new file, 8 MiB chunks by ME_WRITE_THREADS (default 2) threads
void write_bytes_parallel(const std::string& path, const char* data, size_t bytes);
// Buffers that follow the size of each image's file grow in 64 MiB steps, so that a sequence of images settles
inline size_t grow_in_steps(size_t bytes) { return (bytes + ((size_t)64 << 20) - 1) / ((size_t)64 << 20) * ((size_t)64 << 20); }
// The write slots of me_ctx (write-behind): slot k's pinned staging buffer of at least `bytes`; the wait for slot k's pending
// write, whose failure is thrown here ("write-behind: ...")
char* pinned_buf(me_ctx* ctx, size_t bytes, int slot);
void join_pending_write(me_ctx* ctx, int slot);
// A file whose bytes lie in slot `slot`'s pinned buffer, and a small text file written behind it (the .mtl; side_path
// empty: none).  write_pinned_file writes both before it returns, or (behind) starts the slot's thread that does.
struct PinnedFile {
    std::string dest;
    const char* data = nullptr;
    size_t bytes = 0;
    int slot = 0;
    std::string side_path, side_text;
};
void write_pinned_file(me_ctx* ctx, const PinnedFile& file, bool behind);

// calibrate.hip: the two fixed loops of bench.py's calibration leg (out[6])
void calibrate(me_ctx* ctx, double* out);

}  // namespace me

// Every extern "C" entry that takes a context: nothing throws across the boundary.  An me::Error becomes its code and the
// context's last_error; the calling thread's status word is the context's for the kernels that raise bits in it.
#define ME_API_BEGIN(ctx)                      \
    if (!(ctx)) return ME_ERR_BAD_ARG;         \
    try {                                      \
        ME_HIP(hipSetDevice((ctx)->device));   \
        me::set_current_status_word((ctx)->status_dev);

#define ME_API_END(ctx)                                           \
    }                                                             \
    catch (const me::Error& e) {                                  \
        (ctx)->last_error = e.msg;                                \
        return e.code;                                            \
    }                                                             \
    catch (const std::exception& e) {                             \
        (ctx)->last_error = std::string("internal: ") + e.what(); \
        return ME_ERR_BAD_ARG;                                    \
    }                                                             \
    return ME_OK;
