/*
 * matrix_eyes_hip.h — C ABI of libmatrixeyes_hip.so, the MI355X (gfx950) back end for the
 * Depth Pro hot path of zlogic/matrix-eyes.
 *
 * The reference has no FFI seam; its only seam is the compile-time generic `B: Backend`
 * (reference src/reconstruction.rs:155-165, src/depth_pro/mod.rs:251-260).  Every entry point
 * below replaces one Burn-module `forward()` (or one `DepthMap` method) of the reference and
 * cites it.  A Rust caller swaps each `Tensor<B, D>` argument for a `(pointer, dims)` pair;
 * see INTEGRATION.md for the `extern "C"` block and the safe wrapper a maintainer would add.
 *
 * Conventions
 *   - Every function returns an `int32_t` status (ME_OK == 0).  Nothing aborts the process:
 *     shape-invariant violations that `panic!` in the reference (vit.rs:213-218,282,318-324;
 *     decoder.rs:161-165; mod.rs:43-46) come back as ME_ERR_BAD_SHAPE, a missing checkpoint
 *     key (mod.rs:241-243) as ME_ERR_MISSING_WEIGHT.  `me_last_error` gives the text.
 *   - Tensor pointers may be HOST or DEVICE (hipMalloc) addresses; the library asks the HIP
 *     runtime which (hipPointerGetAttributes) and stages host buffers itself.  Layouts are
 *     the reference's: row-major, NCHW for images/feature maps, [B, tokens, C] for token
 *     tensors, f32 elements unless stated.
 *   - A context owns one GPU, one stream, the packed weights and all workspaces; it is used by
 *     one host thread at a time (the reference is single-threaded: reconstruction.rs:61-64).
 *   - No compute entry point has a CPU fallback: without a GPU every one of them fails with
 *     ME_ERR_HIP.
 */
#ifndef MATRIX_EYES_HIP_H
#define MATRIX_EYES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ME_ABI_VERSION 4

/* ---- status codes ------------------------------------------------------------------- */
enum {
    ME_OK = 0,
    ME_ERR_BAD_ARG = 1,        /* null pointer, unknown enum value, bad size            */
    ME_ERR_BAD_SHAPE = 2,      /* the reference's shape panics                          */
    ME_ERR_MISSING_WEIGHT = 3, /* LoaderError::RecorderMissing (mod.rs:241-243)         */
    ME_ERR_BAD_WEIGHT = 4,     /* LoaderError::RecorderErrors: unknown key, wrong shape */
    ME_ERR_HIP = 5,            /* a HIP runtime call or kernel launch failed            */
    ME_ERR_RCCL = 6,           /* an RCCL call failed                                   */
    ME_ERR_IO = 7,             /* OutputError::Io / LoaderError::Pytorch                */
    ME_ERR_NOT_READY = 8,      /* forward called before the weights were finalized      */
    ME_ERR_OOM = 9,            /* device allocation failed                              */
    ME_ERR_OVERFLOW = 10       /* an activation left the f16 operand range (me_status_flags) */
};

/* ---- me_status_flags bits ---------------------------------------------------------------- */
enum {
    ME_STATUS_OVERFLOW_16BIT = 1, /* a kernel rounded a magnitude beyond 65504 to an f16 operand (stored as +-inf) */
    ME_STATUS_SYNC_TIMEOUT = 2    /* a workgroup gave up waiting for its neighbours' LayerNorm statistics (the fused
                                     residual epilogue; needs its sibling workgroups co-resident: a second tenant on
                                     the device's CUs or a CU mask can break that): the step's result is not valid.
                                     The context then falls back to stand-alone LayerNorm launches (me_ln_fusion_state) */
};

/* ---- arithmetic type of the MFMA operands (accumulation is always f32) --------------- */
enum {
    ME_DTYPE_F16 = 0,  /* default: the checkpoint is fp16, so weights are exact          */
    ME_DTYPE_BF16 = 1,
    ME_DTYPE_FP8 = 2   /* BASELINE configs[3]: the ViT linears on MX block-scaled fp8 (e4m3 values, one e8m0
                          scale per 32 K-elements, v_mfma_scale_f32_16x16x128_f8f6f4); everything else f16 */
};

/* ---- element type of a weight tensor handed to me_load_weight ------------------------ */
enum { ME_WEIGHT_F32 = 0, ME_WEIGHT_F16 = 1, ME_WEIGHT_BF16 = 2, ME_WEIGHT_F64 = 3 };

/* ---- which DINOv2 ViT-L of the three in the model (encoder.rs:23-24, fov.rs:25) ------- */
enum { ME_VIT_PATCH_ENCODER = 0, ME_VIT_IMAGE_ENCODER = 1, ME_VIT_FOV_ENCODER = 2 };

/* ---- output.rs:34-38 ------------------------------------------------------------------ */
enum { ME_VERTEX_PLAIN = 0, ME_VERTEX_COLOR = 1, ME_VERTEX_TEXTURE = 2 };

/*
 * Model geometry.  me_default_config() fills in the reference's constants:
 *   vit.rs:17-19,349-358  grid 24 (IMG_SIZE 384 / PATCH_SIZE 16), embed 1024, depth 24, heads 16
 *   encoder.rs:227        taps after blocks 5 and 11
 *   mod.rs:262-263        ENCODER_FEATURE_DIMS [256,512,1024,1024], DECODER_FEATURES 256
 *   mod.rs:308-311        head last_dims [32, 1]
 * Smaller values (grid a multiple of 8, embed a multiple of 64 ...) exist so that parity tests
 * can run the same code on a model the CPU oracle finishes in seconds.  The image side is
 * always 4 * 16 * grid (mod.rs:33) and the merge paddings are grid/8 and grid/4
 * (encoder.rs:267-293 hard-codes 3 and 6 for grid 24).
 */
typedef struct me_model_config {
    int32_t grid;          /* tokens per window side; 24 */
    int32_t embed_dim;     /* 1024 */
    int32_t num_heads;     /* 16; embed_dim / num_heads must be 64 */
    int32_t depth;         /* 24 */
    int32_t tap_blocks[2]; /* {5, 11} */
    int32_t enc_dims[4];   /* {256, 512, 1024, 1024} */
    int32_t dec_dim;       /* 256 */
    int32_t head_dims[2];  /* {32, 1} */
    float ln_eps;          /* Burn LayerNormConfig default 1e-5 (vit.rs:141) */
    int32_t align_corners; /* bilinear pyramid (encoder.rs:128-137): 1 = Burn's historical
                              align_corners=true, 0 = half-pixel centres                  */
    int32_t split_operands; /* bit mask of the stages whose 16-bit activation operands are carried as hi + lo
                               pairs against duplicated weights (2x the MFMA work of that stage, operand
                               rounding 2^-22 instead of 2^-11): 1 = encoder upsample / fuse convs
                               (encoder.rs:307-325), 2 = fusion deconv + out_conv (decoder.rs:95-101), 4 = head
                               (mod.rs:323-333), 8 = decoder.convs (decoder.rs:189-195).  me_default_config: 3
                               (full-size depth error 7.5e-4 relative L2 against the fp32 reference; 0: 1.0e-3,
                               7: 5.8e-4, 15: 5.2e-4 -- DESIGN.md section 5) */
    int32_t fp8_linears;    /* ME_DTYPE_FP8 contexts only: bit mask of the ViT linears that run on MX fp8 -- 1 = qkv,
                               2 = proj, 4 = fc1, 8 = fc2 (vit.rs:60-62,74,120,122); the others stay on the 16-bit kernels.
                               0 = the default ME_FP8_LINEARS_DEFAULT.  profiles/r05_fp8_mask_budget.txt has depth error and
                               time per step for each mask */
} me_model_config;

#define ME_FP8_LINEARS_DEFAULT 13 /* qkv + fc1 + fc2: proj on fp8 buys 0.3 ms for 12 % more depth error */

typedef struct me_ctx me_ctx;

/* progress(user, fraction in [0,1], message-or-NULL): ProgressListener (mod.rs:366-372). */
typedef void (*me_progress_fn)(void* user, float pos, const char* message);

int32_t me_abi_version(void);
int32_t me_default_config(me_model_config* cfg);

/* reconstruction.rs:42-72 init_device + mod.rs:167 DepthProModelLoader::new.
   cfg == NULL means me_default_config. */
int32_t me_ctx_create(int32_t device_id, int32_t dtype, const me_model_config* cfg, me_ctx** out);
void me_ctx_destroy(me_ctx* ctx);
/* Text of the last failure on ctx (ctx == NULL: of the last failed me_ctx_create on this
   thread).  Never NULL. */
const char* me_last_error(const me_ctx* ctx);
int32_t me_ctx_set_progress(me_ctx* ctx, me_progress_fn fn, void* user);
/* Run on a caller-owned hipStream_t (e.g. the framework's current stream) instead of the
   context's own; NULL restores the own stream.  The ordering contract (DESIGN.md "Stream order"):
   every launch, copy and memset of a call with DEVICE pointers is queued on that stream, or on a
   stream of the context forked behind it and joined in front of the call's last launches, so the
   call reads what the caller queued on the stream before it and whatever the caller queues on the
   stream behind it sees its results -- no host wait on either side, eagerly, while the step is
   captured and when it is replayed.  (The first call of a shape allocates its workspaces and waits
   for the stream; later ones do not.)  The call itself waits for the work queued on the stream it
   leaves, and a captured step is dropped: the next call is eager again.  NULL cannot name the
   legacy default stream (handle 0, what a framework calls its default stream): pass a stream the
   caller created.  The caller keeps the stream alive until another one is set or the context is
   destroyed. */
int32_t me_ctx_set_stream(me_ctx* ctx, void* hip_stream);
int32_t me_ctx_synchronize(me_ctx* ctx);
/* Status bits raised by the kernels since the last call (ME_STATUS_*), read and cleared; synchronises the stream.
   The reference computes in f32 (decoder.rs:35-44: relu, conv, adds in f32); this back end rounds MFMA operands to
   16 bit.  An f16 operand holds magnitudes up to 65504: past it the operand is +-inf, and behind a conv + ReLU the
   branch drops out silently.  Every kernel that writes 16-bit operands therefore raises ME_STATUS_OVERFLOW_16BIT
   when that happens.  The word is sticky: no call clears it when it starts.  me_extract_depth[_u8] with a result in
   HOST memory checks it when it has finished, fails with ME_ERR_OVERFLOW itself (also for an overflow that an earlier
   asynchronous call left unread) and clears the bit it reports; with a DEVICE result the call is asynchronous and
   never touches the flag: it stays raised over any number of calls (and graph replays) until the caller asks here.
   bf16 operands (ME_DTYPE_BF16) have f32's range and never raise it.
   ME_STATUS_SYNC_TIMEOUT: a host-result call that meets it runs its step once more on stand-alone LayerNorm launches
   (bit for bit the ME_LN_FUSE=0 result) and succeeds; after device-result calls the NEXT me_extract_depth[_u8] on the
   context fails with ME_ERR_HIP (the earlier depth maps are invalid) and the one after that runs unfused. */
int32_t me_status_flags(me_ctx* ctx, uint32_t* flags);
/* Whether the residual launches of the ViT still carry the LayerNorm behind them (1) or the context has fallen back
   to stand-alone LayerNorm launches (0: after an ME_STATUS_SYNC_TIMEOUT, see above; me_last_error holds the note
   logged then), and how many steps were run again because of it.  Either pointer may be NULL. */
int32_t me_ln_fusion_state(me_ctx* ctx, int32_t* fused, int32_t* fallbacks);

/* ---- weights: mod.rs:174-249 load_record ---------------------------------------------
   Tensors are handed over under their PyTorch checkpoint names and layouts (SURVEY App. C:
   Linear [out,in], Conv2d [out,in,kh,kw], ConvTranspose2d [in,out,kh,kw]); the library
   repacks them for its kernels (the reference's PyTorchToBurnAdapter transposes instead).
   Unknown names and wrong shapes fail like the Applier does (mod.rs:238-240). */
int32_t me_load_weight(me_ctx* ctx, const char* name, const void* data, int32_t weight_dtype,
                       const int64_t* dims, int32_t ndim);
/* Number of tensors the model expects, and the i-th expected name/shape (for loaders). */
int32_t me_expected_weight_count(const me_ctx* ctx);
int32_t me_expected_weight(const me_ctx* ctx, int32_t index, const char** name, int64_t dims[4],
                           int32_t* ndim);
/* Fails with ME_ERR_MISSING_WEIGHT while any expected tensor is absent (mod.rs:241-243). */
int32_t me_weights_finalize(me_ctx* ctx);
/* mod.rs:229-249 load_record for a caller without a PyTorch-checkpoint reader of its own: maps the
   `torch.save` zip archive at `path` (the reference reads it through burn-store's PytorchStore, mod.rs:231),
   loads every tensor the model expects (f16 / f32 / bf16 / f64 storage) and finalizes.  Keys the model does
   not use are skipped, as in the reference, where each part is applied from the full snapshot list and only
   `result.errors` / `result.missing` are checked (mod.rs:236-243); they are listed by
   me_unused_weight_count / me_unused_weight_name.  An unreadable or malformed file is ME_ERR_IO
   (LoaderError::Pytorch), a tensor of the wrong shape ME_ERR_BAD_WEIGHT, an absent one
   ME_ERR_MISSING_WEIGHT. */
int32_t me_load_checkpoint_pt(me_ctx* ctx, const char* path);
int32_t me_unused_weight_count(const me_ctx* ctx);
const char* me_unused_weight_name(const me_ctx* ctx, int32_t index);
/* Size of the packed device weight arena, bytes. */
int64_t me_weight_arena_bytes(const me_ctx* ctx);
/* Device address of the arena, for a caller that moves the packed weights with its own collective
   (e.g. torch.distributed's RCCL communicator) instead of me_bcast_weights; after the bytes have
   arrived on a rank, me_weights_adopt marks every tensor loaded and finalizes. */
void* me_weight_arena_ptr(const me_ctx* ctx);
int32_t me_weights_adopt(me_ctx* ctx);
/* Hash of the arena's layout (dtype, me_model_config, split_operands, every tensor's offset and size).  Contexts
   that exchange arenas must agree on it: me_bcast_weights compares it with rank 0's before the payload moves and
   fails with ME_ERR_BAD_ARG on every rank when one differs; a caller that moves the bytes itself compares it before
   me_weights_adopt. */
uint64_t me_weight_arena_layout(const me_ctx* ctx);

/* ---- the device weight packer and the arena cache (mod.rs:211-247 --convert-checkpoints) ------------------------------
   Who packs a checkpoint tensor into the arena: 0 (the default) the host, one core, with one synchronous upload per
   tensor; 1 the device (csrc/weight_pack.hip): me_load_weight and me_load_checkpoint_pt copy the tensor's raw bytes, in the
   checkpoint's layout and dtype, into a ring of pinned buffers, queue the upload and one pack kernel on the context's
   stream and return; me_weights_finalize waits for them.  The arena is byte for byte the host packer's.  A HOST source is
   not read after me_load_weight returns; a DEVICE source is packed where it lies, by a kernel on the context's stream: its contents
   must be complete when me_load_weight is called (the stream is not ordered behind the caller's) and stay valid and unchanged until
   me_weights_finalize or me_ctx_synchronize.  Any other value is ME_ERR_BAD_ARG. */
int32_t me_ctx_set_weight_packer(me_ctx* ctx, int32_t packer);
/* The arena cache: a 256-byte header (magic, the format constant ME_ARENA_FORMAT of csrc/weight_pack.h, dtype,
   me_model_config, split mask, layout hash, arena size, the source checkpoint's size and mtime, a checksum of the payload
   computed on the device) followed by the raw arena, composed slots included.  me_save_weight_arena writes it for a context
   with finalized weights (ME_ERR_NOT_READY otherwise) to a temporary name beside `path`, then renames; source_path (or
   NULL) names the checkpoint whose stamp is recorded.  me_load_weight_arena reads it into the arena through pinned
   memory, verifies the checksum on the device and finalizes like me_weights_adopt; with source_path the recorded stamp must
   be that file's, if it exists.  A stale file (another stamp or format constant) and a damaged one (short, wrong magic,
   another context's dtype / configuration / layout / size, checksum mismatch) are ME_ERR_IO; after a damaged one the
   context is left unfinalized with every tensor marked not loaded. */
int32_t me_save_weight_arena(me_ctx* ctx, const char* path, const char* source_path);
int32_t me_load_weight_arena(me_ctx* ctx, const char* path, const char* source_path);
/* The cache file's name for a checkpoint: "<dir>/<stem>-<f16|bf16|fp8>-<16 hex digits of me_weight_arena_layout>.mearena".
   Returns its length (buf is NUL-terminated), or -1 for a null argument or a buf that is too small. */
int64_t me_weight_cache_path(const me_ctx* ctx, const char* checkpoint_path, char* buf, int64_t cap);
/* --convert-checkpoints, the policy of both command lines (mod.rs:225-247).  A valid cache file whose checkpoint is absent
   or has the recorded size and mtime is loaded and the checkpoint not opened, whatever `convert` says; a stale one costs
   one line on stderr, the checkpoint is loaded with the selected packer (and the cache rewritten when convert != 0: the
   reference would load the stale file); a damaged one is ME_ERR_IO, the message names the file and says to delete it;
   with no cache file the checkpoint is loaded, and with convert != 0 the cache written afterwards.  *where (or NULL):
   0 the checkpoint with the host packer, 1 with the device packer, 2 the cache. */
int32_t me_load_checkpoint_cached(me_ctx* ctx, const char* checkpoint_path, int32_t convert, int32_t* where);
/* The context's last finished weight load.  info: [0] where the weights came from (as *where above), [1] tensors,
   [2] bytes read, [3] bytes uploaded.  ms: [0] read and stage (host wall clock: the host packer's loops, or the copies into
   the pinned ring), [1] upload, [2] pack kernels (the checksum kernel for the cache) -- HIP event times with the device
   packer and the cache, wall clock with the host packer, [3] compose and finalize, [4] cache write (0: none).
   ME_ERR_NOT_READY before the first load. */
int32_t me_last_weight_load(me_ctx* ctx, int64_t info[4], double ms[5]);

/* ---- multi-GPU start-up: one RCCL broadcast of the packed arena, no collective later ---
   rank 0 finalizes its weights, every rank calls me_bcast_weights with the same 128-byte id
   (from me_rccl_unique_id on rank 0, shipped by the launcher's own store). */
int32_t me_rccl_unique_id(void* id128);
int32_t me_bcast_weights(me_ctx* ctx, const void* id128, int32_t rank, int32_t nranks);

/* ---- forward passes ------------------------------------------------------------------- */

/* reconstruction.rs:114-124: u8 HWC [B,S,S,3] -> f32 NCHW [B,3,S,S], ((x/255)-0.5)/0.5. */
int32_t me_preprocess_u8(me_ctx* ctx, const uint8_t* rgb, int32_t batch, float* img);

/* vit.rs:328-346 DinoVisionTransformer::forward_features.
   xs [W,3,16g,16g]; final_out [W,g*g+1,C] (layer-normed); intermediate_out[i] [W,g*g+1,C]
   (output of block intermediate_blocks[i], not normed).  A requested block that does not
   exist is ME_ERR_BAD_SHAPE (vit.rs:318-324). */
int32_t me_vit_forward_features(me_ctx* ctx, int32_t which_vit, const float* xs, int32_t windows,
                                const int32_t* intermediate_blocks, int32_t n_intermediate,
                                float* final_out, float* const* intermediate_out);

/* encoder.rs:218-335 DepthProEncoder::forward_encodings.  x [B,3,S,S], S = 64*grid;
   encodings[0..4] = [B,dec,S/2,S/2], [B,enc0,S/4,S/4], [B,enc1,S/8,S/8], [B,enc2,S/16,S/16],
   [B,enc3,S/32,S/32]. */
int32_t me_encoder_forward_encodings(me_ctx* ctx, const float* x, int32_t batch,
                                     float* const encodings[5]);

/* decoder.rs:153-208 MultiresConvDecoder::forward: features [B,dec,S/2,S/2],
   lowres_features [B,dec,S/32,S/32]. */
int32_t me_decoder_forward(me_ctx* ctx, const float* const encodings[5], int32_t batch,
                           float* features, float* lowres_features);

/* mod.rs:323-338 head[0..3] + ReLUs: features [B,dec,S/2,S/2] -> canonical inverse depth
   [B,S,S]. */
int32_t me_head_forward(me_ctx* ctx, const float* features, int32_t batch,
                        float* canonical_inverse_depth);

/* fov.rs:40-88 FOVNetwork::forward: x [B,3,S,S], lowres_feature [B,dec,S/32,S/32] ->
   fov_deg [B]. */
int32_t me_fov_forward(me_ctx* ctx, const float* x, const float* lowres_feature, int32_t batch,
                       float* fov_deg);

/* mod.rs:251-363 DepthProModelLoader::extract_depth, for a batch of independent images (the
   reference is batch 1; a batch here equals a loop of batch-1 calls).
   img [B,3,S,S]; f_norm NULL = estimate with the FOV head (mod.rs:343-358), else [B] values;
   inverse_depth [B,S,S] = clamp(canonical / f_norm, 1e-4, 1e4); fov_deg_out NULL or [B]. */
int32_t me_extract_depth(me_ctx* ctx, const float* img, int32_t batch, const float* f_norm,
                         float* inverse_depth, float* fov_deg_out);
/* The same from u8 HWC images, with reconstruction.rs:114-124 fused into the first kernel. */
int32_t me_extract_depth_u8(me_ctx* ctx, const uint8_t* rgb, int32_t batch, const float* f_norm,
                            float* inverse_depth, float* fov_deg_out);
/* The step as one hipGraph (off by default; ME_GRAPH=1 in the environment turns it on at me_ctx_create).  When
   on, a me_extract_depth / me_extract_depth_u8 call whose pointers all name device memory, on a context without a
   progress callback, is enqueued eagerly the first time, captured the second time and replayed with one
   hipGraphLaunch from its third identical invocation on (the shapes are static per batch size).  New weights,
   another stream, batch or pointer start over.  Results are bit-identical to eager launches; the GPU is never
   starved by the host either way, so this buys host CPU time, not depth-maps/s.
   me_graph_launch_count returns the number of replays so far. */
int32_t me_ctx_set_graph(me_ctx* ctx, int32_t on);
int64_t me_graph_launch_count(const me_ctx* ctx);

/* ---- output back end (src/output.rs) -------------------------------------------------- */

/* output.rs:44-75 DepthMap::new clamp to [1/250, 1/0.1] (in place) + inverse_depth_range. */
int32_t me_depth_clamp_minmax(me_ctx* ctx, float* depth, int64_t count, float* min_out,
                              float* max_out);

/* The same without the host round trip: depth and minmax_dev are DEVICE memory, the range {min, max} stays in
   minmax_dev[0..1] for me_stereogram_dev_range / me_depthmap_rgb_dev_range queued behind it on the context's
   stream (DepthMap::new -> output_image chained on the GPU, output.rs:44-75 + :100-121). */
int32_t me_depth_clamp_minmax_async(me_ctx* ctx, float* depth, int64_t count, float* minmax_dev);

/* output.rs:141-193 output_stereogram.  depth [rows,cols] already clamped (DepthMap.data);
   noise [out_h,out_w,3] is the reference's per-row rand stream made an input;
   out [out_h,out_w,3].  Bit-exact with the reference's f32 arithmetic.  rows >= cols is required: the
   reference's sampler reads data[cols * y + x] with x < rows, y < cols (output.rs:79), which leaves a map with
   more columns than rows and panics, so such a map is ME_ERR_BAD_SHAPE here, as are out_w > 16384 and a
   non-positive size (this holds for every stereogram entry below; nothing is written and no file is created).
   A caller-supplied [min_depth, max_depth] narrower than the data must still make every source index
   x + shift - pattern_width land inside the row: the reference panics where it reaches out_w, this library
   clamps it to out_w - 1 silently. */
int32_t me_stereogram(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                      float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                      const uint8_t* noise, uint8_t* out);

/* me_stereogram with the depth range read from device memory (me_depth_clamp_minmax_async). */
int32_t me_stereogram_dev_range(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols,
                                const float* minmax_dev, int32_t out_w, int32_t out_h, float amplitude,
                                const uint8_t* noise, uint8_t* out);

/* ---- keyed stereogram noise (csrc/chacha.h) ------------------------------------------------------- */

/* "Keyed noise" maps a 32-byte key and a size to u8 [out_h,out_w,3]: pixel i = y * out_w + x takes word i & 15 of ChaCha12
   block i >> 4 of the key's stream (64-bit block counter, zero nonce), and R, G, B are the word's three low bytes.  The
   definition is this library's own (it stands in for the reference's rand::rng(), output.rs:163-171, and claims parity with
   no other generator); the kernels and the host twin below share its one text and write the same bytes.

   The key of a seed: eight steps of a 64-bit LCG, one xorshift-rotate output of four little-endian bytes per step.  Needs
   neither a GPU nor a context (ctx-less errors: me_last_error(NULL)); a null pointer is ME_ERR_BAD_ARG. */
int32_t me_noise_key_from_seed(uint64_t seed, uint8_t key[32]);
/* 32 bytes from the operating system (getrandom); a failure of that call is ME_ERR_IO.  No GPU, no context. */
int32_t me_noise_key_from_os(uint8_t key[32]);
/* The CPU twin of me_stereogram_noise on the calling thread: out [out_h,out_w,3] in host memory.  No GPU, no context; a null
   pointer is ME_ERR_BAD_ARG, a non-positive size ME_ERR_BAD_SHAPE. */
int32_t me_stereogram_noise_host(const uint8_t key[32], int32_t out_w, int32_t out_h, uint8_t* out);
/* The noise picture made on the GPU, one ChaCha block per lane: key 32 bytes of HOST memory (it travels as kernel
   arguments); out [out_h,out_w,3], a host or device pointer; enqueued on the context's stream: a device out is not
   synchronised, a host out is.  Sizes as me_stereogram: out_w > 16384 or a non-positive size is ME_ERR_BAD_SHAPE; a null
   key or out is ME_ERR_BAD_ARG.  Needs a context, not finalised weights. */
int32_t me_stereogram_noise(me_ctx* ctx, const uint8_t key[32], int32_t out_w, int32_t out_h, uint8_t* out);
/* me_stereogram with the noise made from `key` on the device: equal, byte for byte, to me_stereogram fed
   me_stereogram_noise_host(key, out_w, out_h), without that buffer existing on the host.  Two launches on the same stream:
   the fill kernel of me_stereogram_noise into context-owned device memory (it grows to the high-water mark), then the
   stereogram kernel (a kernel that made each row's words in place did not beat the pair and was not kept).
   Arguments, refusals and stream as me_stereogram -- a refused call launches nothing; key is HOST memory and travels as
   kernel arguments, so a captured graph replays it. */
int32_t me_stereogram_keyed(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                            float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                            const uint8_t key[32], uint8_t* out);
/* me_stereogram_dev_range with the noise made from `key`. */
int32_t me_stereogram_keyed_dev_range(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols,
                                      const float* minmax_dev, int32_t out_w, int32_t out_h, float amplitude,
                                      const uint8_t key[32], uint8_t* out);
/* The context's last keyed-noise launch.  report: [0] the path taken (1: the fill kernel into the destination of
   me_stereogram_noise; 2: the fill kernel into the context's scratch behind a keyed stereogram entry; there is no fused or
   fallback path), [1] the noise words generated (16 per ChaCha block).  *kernel_ms: the fill kernel's HIP event time.
   Synchronises the context's streams; ME_ERR_NOT_READY before the first such launch. */
int32_t me_last_stereogram_noise(me_ctx* ctx, int64_t report[2], double* kernel_ms);

/* output.rs:123-131 + 633-714 map_depth: depth [count] -> rgb [count,3] (before the Lanczos
   resize, which is the identity at the native size). */
int32_t me_depthmap_rgb(me_ctx* ctx, const float* depth, int64_t count, float min_depth,
                        float max_depth, uint8_t* rgb);

/* me_depthmap_rgb with the depth range read from device memory (me_depth_clamp_minmax_async). */
int32_t me_depthmap_rgb_dev_range(me_ctx* ctx, const float* depth, int64_t count, const float* minmax_dev,
                                  uint8_t* rgb);

/* ---- Lanczos3 resampling (the `image` crate's imageops::resize, FilterType::Lanczos3) ---------------------- */

/* Largest width or height, in or out, that the resampler accepts (index arithmetic is 64-bit; the f32
   intermediate of w * nh * 3 floats is the context's scratch: 3 GiB at 16384 x 16384). */
#define ME_RESIZE_MAX_DIM 16384

/* reconstruction.rs:107-113, output.rs:133-137, output.rs:206-218: DynamicImage::resize_exact(nw, nh, Lanczos3)
   for 8-bit RGB: src [h,w,3] -> dst [nh,nw,3], byte for byte what the crate (0.25.10, imageops/sample.rs) writes:
   vertical pass into an unclamped f32 intermediate, horizontal pass, round(clamp(t, 0, 255)); the same size in and
   out is a copy.  Host or device pointers; enqueued on the context's stream: a device dst is not synchronised, a
   host dst is.  Needs a context, not finalised weights.  Chained with me_extract_depth_u8 on a device dst this is
   the photo path of reconstruction.rs:107-124.  src and dst overlapping (or equal) is ME_ERR_BAD_ARG; a
   non-positive size or one above ME_RESIZE_MAX_DIM is ME_ERR_BAD_SHAPE.  Scratch (the staged source, the
   intermediate, the per-axis weight tables) belongs to the context and grows to the high-water mark. */
int32_t me_resize_lanczos3_rgb8(me_ctx* ctx, const uint8_t* src, int32_t w, int32_t h,
                                uint8_t* dst, int32_t nw, int32_t nh);

/* output.rs:123-139 output_depth_map up to the save: the colour map into RgbImage::new(data_width, data_height),
   filled in data order (:124-131), then the resize to the original size (:133-137).  depth [data_height,data_width]
   is DepthMap.data; rgb [out_h,out_w,3].  minmax_dev NULL: the two scalars are used; else the range
   me_depth_clamp_minmax_async left on the device (min_depth / max_depth ignored).  Pointers, stream and errors as
   me_resize_lanczos3_rgb8. */
int32_t me_depthmap_rgb_resized(me_ctx* ctx, const float* depth, int32_t data_width, int32_t data_height,
                                float min_depth, float max_depth, const float* minmax_dev,
                                int32_t out_w, int32_t out_h, uint8_t* rgb);

/* ---- PNG encoding on the device (RgbImage::save to ".png") ---------------------------------------------------------- */

/* RgbImage::save to ".png" (output.rs:138, :192): rgb [h,w,3] -> a complete PNG file (colour type 2, bit depth 8, no
   interlace; adaptive row filters, one dynamic-Huffman or stored deflate chunk per 64 KiB of filtered rows, one IDAT per
   chunk) in DEVICE memory owned by the context (valid until its next PNG call); host or device rgb; enqueued on the
   context's stream, synchronised because it returns a size.  Any decoder reads the file back to exactly the input
   pixels; its bytes are this encoder's own (a pure function of the pixels), not the `png` crate's.  Needs a context, not
   finalised weights.  A null pointer is ME_ERR_BAD_ARG; a non-positive size or one above ME_RESIZE_MAX_DIM is
   ME_ERR_BAD_SHAPE.  Scratch belongs to the context and grows to the high-water mark. */
int32_t me_png_encode_rgb8(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h,
                           const uint8_t** png_dev, int64_t* nbytes);
/* The same, copied to the host once and written to destination_path (an unwritable path is ME_ERR_IO). */
int32_t me_output_png(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, const char* destination_path);
/* output.rs:123-139 output_depth_map, whole: me_depthmap_rgb_resized into context-owned device memory, then
   me_output_png.  Arguments and errors as me_depthmap_rgb_resized. */
int32_t me_output_depth_map_png(me_ctx* ctx, const float* depth, int32_t data_width, int32_t data_height,
                                float min_depth, float max_depth, const float* minmax_dev,
                                int32_t out_w, int32_t out_h, const char* destination_path);
/* output.rs:141-193 output_stereogram, whole: me_stereogram into context-owned device memory, then me_output_png.
   Arguments and errors as me_stereogram. */
int32_t me_output_stereogram_png(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                 float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                 const uint8_t* noise, const char* destination_path);
/* The same with the noise made from `key` (me_stereogram_keyed): arguments, refusals and stream as me_output_stereogram_png. */
int32_t me_output_stereogram_png_keyed(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                       float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                       const uint8_t key[32], const char* destination_path);

/* ---- JPEG encoding on the device (RgbImage::save to ".jpg" / ".jpeg") -------------------------------------------------- */

/* RgbImage::save to ".jpg" (output.rs:138, :192): rgb [h,w,3] -> a complete baseline JFIF file (SOF0, 8 bits, three
   components in one interleaved scan, the Annex K quantisation tables scaled by `quality` and the Annex K Huffman tables,
   no restart markers) in DEVICE memory owned by the context (valid until its next JPEG-encode call); host or device rgb;
   enqueued on the context's stream, synchronised because it returns a size.  quality is 1..100; subsampling 0 = 4:4:4,
   1 = 4:2:2, 2 = 4:2:0.  The bytes are those libjpeg writes for the same parameters with its integer DCT and optimize off
   (Pillow's Image.save(.., "JPEG", quality=, subsampling=, optimize=False)), and those of the C++ host layer's encode_jpeg.
   Needs a context, not finalised weights.  A null pointer, a quality outside 1..100 or a subsampling outside 0..2 is
   ME_ERR_BAD_ARG; a non-positive size or one above min(ME_RESIZE_MAX_DIM, 65535) is ME_ERR_BAD_SHAPE.  Scratch belongs to
   the context and grows to the high-water mark. */
int32_t me_jpeg_encode_rgb8(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, int32_t quality, int32_t subsampling,
                            const uint8_t** jpg_dev, int64_t* nbytes);
/* The same, copied to the host once and written to destination_path (an unwritable path is ME_ERR_IO). */
int32_t me_output_jpeg(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, int32_t quality, int32_t subsampling,
                       const char* destination_path);
/* output.rs:123-139 output_depth_map to a ".jpg" destination, whole: me_depthmap_rgb_resized into context-owned device
   memory, then me_output_jpeg.  Arguments and errors as me_depthmap_rgb_resized and me_output_jpeg. */
int32_t me_output_depth_map_jpeg(me_ctx* ctx, const float* depth, int32_t data_width, int32_t data_height,
                                 float min_depth, float max_depth, const float* minmax_dev,
                                 int32_t out_w, int32_t out_h, int32_t quality, int32_t subsampling,
                                 const char* destination_path);
/* output.rs:141-193 output_stereogram to a ".jpg" destination, whole: me_stereogram into context-owned device memory, then
   me_output_jpeg.  Arguments and errors as me_stereogram and me_output_jpeg. */
int32_t me_output_stereogram_jpeg(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                  float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                  const uint8_t* noise, int32_t quality, int32_t subsampling,
                                  const char* destination_path);
/* The same with the noise made from `key` (me_stereogram_keyed): arguments, refusals and stream as
   me_output_stereogram_jpeg. */
int32_t me_output_stereogram_jpeg_keyed(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                        float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                        const uint8_t key[32], int32_t quality, int32_t subsampling,
                                        const char* destination_path);

/* ---- JPEG decoding on the device (reconstruction.rs:95-113: ImageReader::open(..).decode(), apply_orientation) --------- */

/* Frame size and EXIF span of a JPEG file in memory: width / height as coded (before any orientation), and the offset and
   length inside `file` of the TIFF-structured EXIF block (behind "Exif\0\0" of the first APP1 segment that has one; 0, 0:
   none), which the caller parses with what it has.  Needs neither a GPU nor a context (ctx-less errors: me_last_error(NULL)).
   A null pointer is ME_ERR_BAD_ARG, and so is a file the decoder refuses, with the decoder's message. */
int32_t me_jpeg_info(const uint8_t* file, int64_t nbytes, int32_t* width, int32_t* height,
                     int64_t* exif_offset, int64_t* exif_nbytes);
/* The picture of a JPEG file (baseline, extended sequential or progressive Huffman; 8 bits; grey or three components with
   integer sampling ratios; restart intervals), byte for byte what the C++ host layer's decoder writes (host/jpeg_decoder.cpp
   decode_jpeg) followed by apply_orientation(orientation): the entropy-coded segments are decoded on the host into
   pinned memory, and dequantisation, IDCT, level shift, chroma upsampling, colour conversion and the orientation run on the
   GPU.  rgb [h,w,3] is the ORIENTED size (w and h swap for orientations 5..8), a host or device pointer; enqueued on the
   context's stream: a device rgb is not synchronised, a host rgb is (the convention of me_resize_lanczos3_rgb8).  A null
   pointer or an orientation outside 1..8 is ME_ERR_BAD_ARG; a size that does not match the file ME_ERR_BAD_SHAPE; a file
   the decoder refuses ME_ERR_BAD_ARG with the decoder's own message ("<jpeg>: ..." in place of a path).  Needs a
   context, not finalised weights.  Scratch belongs to the context and grows to the high-water mark. */
int32_t me_jpeg_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation,
                            uint8_t* rgb, int32_t w, int32_t h);
/* reconstruction.rs:95-113 in one call: me_jpeg_decode_rgb8 into context-owned device memory, then
   me_resize_lanczos3_rgb8 to dst [nh,nw,3] (host or device): only the resized picture can cross to the host.  Errors as
   the two calls; the oriented picture's sides are bound by ME_RESIZE_MAX_DIM. */
int32_t me_jpeg_decode_resized_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation,
                                    uint8_t* dst, int32_t nw, int32_t nh);
/* Legs of the context's last JPEG decode in milliseconds: [0] entropy decoding on the host (wall clock), [1] upload of the
   coefficients, [2] jpeg_idct_kernel, [3] jpeg_finish_kernel, [4] download to a host rgb (0 for a device one); [1]..[4]
   are HIP event times.  Synchronises the context's stream. */
int32_t me_last_jpeg_timing(me_ctx* ctx, double ms_out[5]);
/* Where me_jpeg_decode_rgb8 / me_jpeg_decode_resized_rgb8 decode the entropy-coded data: 0 (the default) on the host, as
   described above; 1 on the device (csrc/jpeg_entropy.hip): the scan's bytes go up instead of the coefficients and are
   Huffman-decoded by one thread per subsequence of bits, with the host decoder's coefficients integer for integer, so the
   picture's bytes do not change.  The device decoder takes sequential files (SOF0 / SOF1) with ONE scan that holds all
   components, prefix-code Huffman tables, DC categories up to 15, no marker but RSTn inside the scan and all the RSTn the
   restart interval needs; progressive and multi-scan files, and a file whose true chain meets an invalid code, a run past
   coefficient 63, a segment that ends early or no synchronisation within 65536 bits, are DECLINED: the host decoder then
   runs whole, so the picture or the refusal is the host's either way.  Any other mode is ME_ERR_BAD_ARG. */
int32_t me_ctx_set_jpeg_entropy(me_ctx* ctx, int32_t mode);
/* The entropy leg of the context's last JPEG decode.  report: [0] where the coefficients were made (0 host, 1 device),
   [1] why the device declined (0: it did not, or was not asked; 1 progressive, 2 scans, 3 Huffman table not a prefix code,
   4 DC value above 15, 5 marker inside the scan, 6 too few RSTn, 7 MCU / scan too large, 8 the planner refused the file,
   10 invalid code, 11 run past 63, 12 no synchronisation, 13 segment ends early), [2] segments (restart intervals),
   [3] subsequences, [4] bits per subsequence, [5] synchronisation rounds, the confirming one included, [6] bytes uploaded,
   [7] workgroups of each entropy kernel.  ms: [0] marker scan and destuffing on the host (wall clock), [1] upload,
   [2] entropy kernels with the looks at their changed counts (HIP events). */
int32_t me_last_jpeg_entropy(me_ctx* ctx, int64_t report[8], double ms[3]);

/* ---- PNG decoding on the device (reconstruction.rs:95-113 for the photo, output.rs:206-218 for vertex colours) ---------- */

/* Size and EXIF span of a PNG file in memory: width / height of IHDR (before any orientation), and the offset and length
   inside `file` of the body of the last eXIf chunk (the TIFF-structured block; 0, 0: none), which the caller parses with
   what it has.  Needs neither a GPU nor a context (ctx-less errors: me_last_error(NULL)).  A null pointer is
   ME_ERR_BAD_ARG, and so is a file whose chunks or header the decoder refuses, with the decoder's message. */
int32_t me_png_info(const uint8_t* file, int64_t nbytes, int32_t* width, int32_t* height,
                    int64_t* exif_offset, int64_t* exif_nbytes);
/* The picture of a PNG file (every colour type and bit depth of the specification's table 11.1, interlaced or not; alpha
   dropped, 16-bit samples rounded to 8, as DynamicImage::into_rgb8 does), byte for byte what the C++ host layer's decoder
   writes (host/png_decoder.cpp decode_png) followed by apply_orientation(orientation).  The host inflates the IDAT data
   into pinned memory band by band; every finished band of rows is copied up and its unfilter launch queued behind it, so
   the GPU works under the inflate; the conversion to RGB, the de-interlacing and the orientation are one more kernel.
   rgb [h,w,3] is the ORIENTED size (w and h swap for orientations 5..8), a host or device pointer; enqueued on the
   context's stream: a device rgb is not synchronised (except for a palette file, whose index check comes back from the
   device), a host rgb is.  A null pointer or an orientation outside 1..8 is ME_ERR_BAD_ARG; a size that does not match the
   file ME_ERR_BAD_SHAPE; a file the decoder refuses ME_ERR_BAD_ARG with the host decoder's own message ("<png>: ..." in
   place of a path): when the device path meets a defect the host decoder runs whole and its words stand.  On an error
   the destination's contents are unspecified and the context stays usable.  Needs a context, not finalised weights.
   Scratch belongs to the context and grows to the high-water mark. */
int32_t me_png_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation,
                           uint8_t* rgb, int32_t w, int32_t h);
/* reconstruction.rs:95-113 in one call: me_png_decode_rgb8 into context-owned device memory, then
   me_resize_lanczos3_rgb8 to dst [nh,nw,3] (host or device): only the resized picture can cross to the host.  Errors as
   the two calls; the picture's sides are bound by ME_RESIZE_MAX_DIM. */
int32_t me_png_decode_resized_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation,
                                   uint8_t* dst, int32_t nw, int32_t nh);
/* Legs of the context's last PNG decode in milliseconds: [0] inflate on the host (wall clock; the uploads and launches
   are queued from inside it), [1] uploads of the bands, [2] png_unfilter_kernel launches, [3] png_finish_kernel,
   [4] download to a host rgb (0 for a device one); [1]..[4] are HIP event times, summed over the bands.  Synchronises the
   context's stream. */
int32_t me_last_png_timing(me_ctx* ctx, double ms_out[5]);

/* output.rs:264-363 IndexedMesh::new + for_each_face + remap_face.
   depth [height,width] (DepthMap.data, stride `width`).  vertex_index [height*width]: the
   first-use vertex id or -1.  faces [nfaces,3] remapped vertex ids in the reference's
   emission order; faces may be NULL to only count, else it needs room for
   2*(width-1)*(height-1) triangles. */
int32_t me_mesh_index(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                      int32_t* vertex_index, int64_t* nvertices, int64_t* nfaces, int32_t* faces);

/* output.rs:228-249: per vertex id (sorted_vertices order) uv [nvertices,2] = (x/w, y/h) and
   xyz [nvertices,3] = (xm*(xn-0.5)*z, ym*(yn-0.5)*z, z), z = 1/depth, before the writer's
   sign flips.  vertex_index comes from me_mesh_index. */
int32_t me_mesh_vertices(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                         const int32_t* vertex_index, int64_t nvertices, uint32_t original_width,
                         uint32_t original_height, float* uv, float* xyz);

/* output.rs:100-112 + 195-261 output_mesh with ObjWriter (:484-630) / PlyWriter (:385-482):
   indexes the mesh on the GPU and writes `destination_path` (".obj", ".ply" or ".glb", case-insensitive,
   anything else is ME_ERR_BAD_ARG; for ".obj" in texture mode also "<stem>.mtl" next to it).
   ".glb" is not a format of the reference's: a glTF 2.0 binary mesh, described at me_mesh_glb_bytes.
   depth [height,width] is DepthMap.data (already clamped).  vertex_colors: NULL, or u8
   [height*width,3] = the source image resized to the depth map (only read in ME_VERTEX_COLOR
   mode; me_resize_lanczos3_rgb8 makes it, output.rs:206-218). Text output is byte-identical to
   the reference's: numbers are printed like Rust's `{}` for f64 (shortest round-trip, never
   scientific). */
int32_t me_output_mesh(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                       uint32_t original_width, uint32_t original_height,
                       const char* destination_path, const char* source_path, int32_t vertex_mode,
                       const uint8_t* vertex_colors);

/* Write-behind for me_output_mesh(".obj", ".ply" and ".glb") (BASELINE configs[4]: a batch of images, each ending in a
   file of 70 - 450 MB; a .glb of up to 94 MB).  files_in_flight >= 2: the call returns once the file's bytes sit in pinned host memory; a host thread
   writes the file (and an OBJ's .mtl) while the caller goes on to the next image.  That many pinned buffers are used in turn, so that many files
   can be in flight; the next call waits for the oldest (1 is taken as 2) -- and for any pending write to its own
   destination path -- before it starts any work of its own.  A failed write is reported (ME_ERR_IO, me_last_error) by
   the call that next waits for it: a later me_output_mesh (which then has written nothing and can be repeated),
   me_ctx_set_write_behind, or me_output_flush, which waits for every pending file.  me_ctx_destroy flushes.  0 (the default): the reference's
   form, output_mesh returns with the file written. */
int32_t me_ctx_set_write_behind(me_ctx* ctx, int32_t files_in_flight);
/* Output overlap (BASELINE configs[4]; reconstruction.rs:155-205 runs extract_depth -> DepthMap::new -> output_image per
   image, one after the other): with on = 1 every output back-end call of this section that reads a DEVICE depth buffer
   runs on a second stream of the context, ordered behind the me_extract_depth[_u8] call that WROTE that buffer (known by
   its address) instead of behind everything queued since.  A caller that alternates two device depth buffers can
   therefore queue image i + 1's me_extract_depth first and then make image i's output calls: the GPU works on the next
   depth map while the host waits for this image's mesh counts, OBJ text and its copy to the host.  The next
   me_extract_depth that writes a buffer waits (on the GPU) for the output calls still reading it.  me_ctx_synchronize
   and me_output_flush wait for both streams.  Results are unchanged.  0 (the default): one stream, the reference's order.
   The ordering contract with on = 1 (also on a caller's stream, me_ctx_set_stream): an output call reads its inputs
   behind the step that wrote the depth buffer or, for a buffer no step of this context wrote, behind everything queued
   on the context's stream when the call is made, and output calls follow one another; but what they WRITE to device
   memory (me_depth_clamp_minmax_async's range, a device rgb / stereogram) is written on the second stream, which the
   context's stream is NOT ordered behind: work the caller queues behind the call does not see it.  The caller reads such
   a result after me_ctx_synchronize or me_output_flush, and only a later output call of this context may consume it
   without that wait.  With on = 0 the results are ordered on the context's stream like any other call's. */
int32_t me_ctx_set_output_overlap(me_ctx* ctx, int32_t on);
int32_t me_output_flush(me_ctx* ctx);

/* The OBJ text of me_output_mesh without the file: the mesh is indexed and every "vt" / "v" / "f" line formatted on
   the GPU (output.rs:484-630 ObjWriter; numbers as Rust's `{}` prints an f64), the lines packed in the reference's
   order behind the "mtllib <stem>.mtl" / "usemtl Textured" header of texture mode.  *text_dev: DEVICE address of the
   bytes, owned by the context and valid until its next mesh call; *nbytes: their count.  me_output_mesh(".obj") is
   this text copied to the host once and written to the file. */
int32_t me_mesh_obj_text(me_ctx* ctx, const float* depth, int32_t width, int32_t height, uint32_t original_width,
                         uint32_t original_height, const char* stem, int32_t vertex_mode,
                         const uint8_t* vertex_colors, const uint8_t** text_dev, int64_t* nbytes);

/* The PLY file of me_output_mesh without the file: the mesh is indexed and its binary records packed on the GPU
   (output.rs:385-482 PlyWriter: x, -y, -z as big-endian f64 and, in ME_VERTEX_COLOR mode with vertex_colors, r g b per
   vertex; the byte 3 and three big-endian u32 ids per face) behind the ASCII header.  *bytes_dev: DEVICE address, owned
   by the context, valid until its next mesh call; *nbytes: the size of the file.  me_output_mesh(".ply") is these
   bytes copied to the host once and written to the file. */
int32_t me_mesh_ply_bytes(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                          uint32_t original_width, uint32_t original_height, int32_t vertex_mode,
                          const uint8_t* vertex_colors, const uint8_t** bytes_dev, int64_t* nbytes);

/* The glTF 2.0 binary file of me_output_mesh(".glb") without the file.  A 12-byte header, one JSON chunk padded with
   spaces to a length that is 4 mod 16, and one BIN chunk, whose payload therefore starts at a multiple of 16 in the
   file.  BIN holds, each at a multiple of 16 with zeros between: the positions, nvertices x 3 little-endian f32
   (x, -y, -z: the sign flips of the reference's writers, output.rs:450, and glTF's camera convention); in
   ME_VERTEX_COLOR mode with vertex_colors, nvertices x (r, g, b, 255) u8 (without them no colour section and no COLOR_0,
   as the PLY records fall back to 24 bytes); in ME_VERTEX_TEXTURE mode nvertices x 2 f32, the uv of me_mesh_vertices
   unchanged (glTF's v runs downwards), and a material whose texture is the image {"uri": source_path}, JSON-escaped
   but otherwise as given (the string the .mtl has behind map_Kd: relative to the caller's directory, not embedded);
   then the faces as 3 x nfaces little-endian u32 in the reference's emission order.  The position accessor's min / max
   are the exact f32 bounds of the written values, reduced on the GPU and printed as the OBJ writer prints a number.
   An empty mesh is a valid asset with no geometry and no BIN chunk.  ME_ERR_BAD_ARG, nothing written: a bound that is
   not finite (JSON cannot hold it), a file of 2^32 bytes or more.  *bytes_dev: DEVICE address, owned by the context,
   valid until its next mesh call; *nbytes: the size of the file.  me_output_mesh(".glb") is these bytes copied to the
   host once and written to the file. */
int32_t me_mesh_glb_bytes(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                          uint32_t original_width, uint32_t original_height, const char* source_path,
                          int32_t vertex_mode, const uint8_t* vertex_colors, const uint8_t** bytes_dev,
                          int64_t* nbytes);

/* Where the last me_output_mesh(".obj", ".ply" or ".glb") call on this context spent its time, host wall clock in milliseconds:
   ms_out[0] mesh indexing + vertex kernels (incl. their read-back of the counts), [1] the kernels that format the OBJ
   text, pack the PLY records or pack the GLB sections (the read-back of the GLB's position bounds included), [2] the D2H copy of the file's bytes into pinned memory, [3] the file write (the host
   kernel's page-cache copy; with write-behind, the hand-over to the writing thread); *text_bytes (optional): the size
   of the file.  (A call served by a host serialiser -- ME_OBJ_HOST_FORMAT, ME_PLY_HOST_FORMAT, ME_GLB_HOST_FORMAT -- is not reported.) */
int32_t me_last_mesh_timing(const me_ctx* ctx, double ms_out[4], int64_t* text_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MATRIX_EYES_HIP_H */
