// Internal declarations shared by the HIP translation units of libmatrixeyes_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/matrix_eyes_hip.h"
#include "error.h"        // Error, fail, ME_CHECK
#include "gemm_params.h"  // Act, GemmParams, RowSegs and their builders: whatever a launch is described in
#include "tile_choice.h"  // AMode, EpiKind, CFG_*, cdiv, seg_row_tiles: whatever a launch decision is stated in

namespace me {

typedef _Float16 f16;
typedef __bf16 bf16;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((__vector_size__(8)));

struct Status {
    int32_t code = ME_OK;
    std::string msg;
};

#define ME_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            ::me::fail(e__ == hipErrorOutOfMemory ? ME_ERR_OOM : ME_ERR_HIP, "%s: %s (%s:%d)", \
                       #expr, hipGetErrorString(e__), __FILE__, __LINE__);                   \
    } while (0)

// Environment knobs: a switch that is on unless NAME=0, one that is off unless NAME is a non-zero number, a
// number with a default.  Whether a knob is read once per process (`static const` at the site) or per call is the site's choice.
static inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline bool env_on(const char* name) { return env_int(name, 1) != 0; }
static inline bool env_flag(const char* name) { return env_int(name, 0) != 0; }

// Per-kernel launch configuration that must be set up once PER DEVICE (dynamic-LDS attribute, resident
// workgroup count): contexts may live on several devices, and on several host threads, of one process.
constexpr int kMaxDevices = 64;
struct PerDeviceOnce {
    std::atomic<int> value[kMaxDevices];
    PerDeviceOnce() {
        for (auto& v : value) v.store(0, std::memory_order_relaxed);
    }
};
// value cached for the current device (0 = not configured yet); `configure` returns the value to cache (> 0).
// Two threads racing on the same device both configure (idempotent HIP calls) and store the same value.
template <typename F>
static inline int per_device_once(PerDeviceOnce& once, F&& configure) {
    int dev = 0;
    ME_HIP(hipGetDevice(&dev));
    ME_CHECK(dev >= 0 && dev < kMaxDevices, ME_ERR_BAD_ARG, "device ordinal %d out of range", dev);
    int v = once.value[dev].load(std::memory_order_acquire);
    if (!v) {
        v = configure(dev);
        once.value[dev].store(v, std::memory_order_release);
    }
    return v;
}

// ---------------------------------------------------------------------------------------
// Optional per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).
// Off by default; when on, every instrumented launch is bracketed by two events.
// ---------------------------------------------------------------------------------------
struct ProfEntry {
    std::string name;
    double flops, bytes;
    hipEvent_t e0, e1;
};
struct Profiler {
    bool enabled = false;
    std::vector<ProfEntry> entries;
};
Profiler& profiler();
struct ProfScope {
    hipStream_t stream;
    int index = -1;
    ProfScope(hipStream_t s, const std::string& name, double flops, double bytes);
    ~ProfScope();
};

// ---------------------------------------------------------------------------------------
// 16-bit operand overflow guard.  An f16 operand holds magnitudes up to 65504; past it the stored operand is
// +-inf, and on a conv stage infinities of both signs sum to NaN which the ReLU behind maps to 0 -- the branch
// drops out silently, where the fp32 reference (decoder.rs:35-44) has no such limit.  Every kernel that rounds f32
// values to f16 operands keeps the largest magnitude it stored and raises bit ME_STATUS_OVERFLOW_16BIT of the
// calling context's status word when it exceeds 65504 (one atomicOr on the rare path).
// The word of the context whose entry point is running on this host thread (set by ME_API_BEGIN).
// ---------------------------------------------------------------------------------------
unsigned* current_status_word();
void set_current_status_word(unsigned* w);
#if defined(__HIPCC__)
template <typename T>
__device__ __forceinline__ void raise_overflow16(unsigned* status, float amax) {
    if constexpr (sizeof(T) == 2 && !__is_same(T, bf16)) {
        if (status && amax > 65504.0f) atomicOr(status, 1u);
    }
}
#endif

// ---------------------------------------------------------------------------------------
// Device helpers shared by the GEMM and attention kernels.
// ---------------------------------------------------------------------------------------
// 16-byte LDS-DMA: lane l's 16 bytes at gsrc land at lds_base + 16 l (M0 carries the wave-uniform base).
// LDS-DMA issued behind the compiler's back (two-group and ring GEMM kernels, attention).  The waitcnt pass orders every
// later LDS access behind a builtin LDS-DMA with vmcnt(0), which would serialise exactly what that kernel
// overlaps; issued as asm the DMA is invisible to it and the kernel places its own counted waits.  The
// compiler's own vmcnt waits stay safe: an unknown extra VMEM operation in flight can only make a counted
// wait longer (returns are in order).  lds_base: wave-uniform LDS byte address; lane l writes base + 16 l.
// Address = uniform 64-bit base (SGPR pair) + 32-bit per-lane byte offset: no address VALU, half the
// address registers.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is "reserved": the kernel has no other user of it
__device__ __forceinline__ void glds16_raw(const void* sbase, unsigned voff, unsigned lds_base) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :
                 : "v"(voff), "s"(sbase), "s"(lds_base)
                 : "memory", "m0");
}
#pragma clang diagnostic pop
// a pointer the compiler may hold in VGPRs although every lane has the same value -> SGPR pair
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const char*)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ unsigned lds_address(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}

// s_waitcnt vmcnt(N) with a compile-time N (gfx9 encoding: vmcnt in bits 3:0 and 15:14)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// ---------------------------------------------------------------------------------------
// GEMM / implicit-GEMM convolution: D[m][n] = sum_k A(m,k) * W[n][k]  (+ epilogue).
// W is always row-major [N][K], K contiguous (the PyTorch Linear layout; conv weights are
// repacked to [Cout][tap][Cin] at load time).
// ---------------------------------------------------------------------------------------
// AMode (A_PLAIN / A_CONV) and EpiKind (EPI_*): tile_choice.h.  Act, GemmParams and its builders: gemm_params.h.  What a launcher
// refuses before it launches: admission.h

// Tile configurations of gemm_launch: the CFG_* ids, what each is and admits, and every rule that picks one live in tile_choice.h.
// The knobs those rules read, as the environment had them when the process first asked (gemm.hip).
const TileKnobs& tile_knobs();
// dtype: ME_DTYPE_F16 / ME_DTYPE_BF16.  Picks a tile configuration from (M, N, K) unless force_cfg names one.
void gemm_launch(const GemmParams& p, AMode amode, EpiKind epi, int32_t dtype, hipStream_t stream,
                 int32_t force_cfg = -1);
// The depth head's final 3x3 (128 -> 32) + 1x1 (32 -> 1) on a pixel halo tile with the weights held in registers
// (head_conv.hip); gemm_launch takes it for EPI_HEAD_FINAL where the shape fits (ME_HEAD_HALO=0: the implicit-GEMM tile)
bool head_final_halo_fits(const GemmParams& p);
// the head's ConvTranspose + conv3x3 + ReLU + conv1x1 + ReLU + / f_norm + clamp as ONE launch on the half-resolution map
// (gemm_*_conv.hip: the 128-channel halo tile with the EPI_HEAD_COMPOSED epilogue).  p: A = bordered [B][H+2][W+2][Cin] 16-bit,
// W = composed [128][9][Cin], bias = f32 [32], tap_bias = f32 [9][32], w2 / b2 / f_norm / clamp / pixels_per_image (of the
// FULL-resolution map) as for EPI_HEAD_FINAL, out32 = depth [B][2H][2W]
void head_composed_launch(const GemmParams& p, int32_t dtype, hipStream_t stream);  // (what fits: admission.h head_composed_fits)
// compute units `stream` may use: the bits of its CU mask (hipExtStreamGetCUMask), the device's count when the stream
// has no mask or the runtime cannot say
int stream_cu_count(hipStream_t stream);
// workgroups of the fused residual + LayerNorm launch (gemm_core.h resid_ln_epilogue) that are resident at once on
// the CUs `stream` may use; a launch with N columns needs 8 * N / 256 of them (one row tile per XCD with all its column
// tiles: they wait for one another)
int gemm_lnf_resident(int32_t dtype, hipStream_t stream);
int gemm_fp8_lnf_resident(hipStream_t stream);  // ... of the kernel an fp8 proj / fc2 carries it in (gemm_fp8.hip gemm_pp8t_kernel<.., LNF>)
// test knobs of the two-group launchers, read once per process (gemm.hip): ME_GEMM_GRID_LIMIT (0: none), ME_LN_SPIN_LIMIT (0: the kernel's bound)
int gemm_grid_limit();
int gemm_ln_spin_limit();
void head_final_halo_launch(const GemmParams& p, int32_t dtype, hipStream_t stream);

// MX fp8 x fp8 (gemm_fp8.hip): EPI_STORE (f16 out16, or fp8 out8 + scales) / EPI_RESID_SCALE
void gemm_fp8_launch(const GemmParams& p, EpiKind epi, hipStream_t stream);
// f16 [rows][K] -> e4m3 + e8m0 scales in the weight (1) or activation (0) scale layout
void quantize_f16_to_fp8_launch(const void* src16, uint8_t* dst8, uint8_t* scales, int64_t rows, int32_t K,
                                int32_t weight_layout, hipStream_t stream);
int gemm_num_configs();
const char* gemm_config_name(int cfg);

// ---------------------------------------------------------------------------------------
// Attention: qkv [rows][3*C] (q | k | v, each [heads][64]), rows = windows * tokens;
// out [rows][C].  softmax(q*scale . k^T) v per (window, head); head_dim is 64.
// ---------------------------------------------------------------------------------------
// RowSegs (the row segments of the encoder's merged ViT launches) and kAttnQScale: gemm_params.h
// out8 != nullptr: the output is written as MX fp8 bytes [rows][C] + activation-layout block scales (mx_fp8.h,
// out8_mt = 128-row tiles of the operand) instead of 16-bit `out`
void attention_launch(const void* qkv, void* out, int32_t windows, int32_t tokens, int32_t heads,
                      int32_t dtype, hipStream_t stream, const RowSegs* segs = nullptr, uint8_t* out8 = nullptr,
                      uint8_t* out8_scale = nullptr, int64_t out8_mt = 0, bool q_prescaled = false);
// attention3.hip: a development re-cut (48 queries per wave on 16x16x32 MFMAs, the query beyond whole wave units on the vector
// pipe) that attention_launch reaches only with ME_ATT_V=3; for a pre-scaled Q it runs attention.hip's attention2_kernel
void attention3_launch(const void* qkv, void* out, int32_t windows, int32_t tokens, int32_t heads, int32_t dtype, hipStream_t stream,
                       const RowSegs& segs, uint8_t* out8, uint8_t* out8_scale, int64_t out8_mt, float defer_thr);

// ---------------------------------------------------------------------------------------
// Row-wise and layout kernels (elementwise.hip)
// ---------------------------------------------------------------------------------------
// y16[r][:] = (x[r][:] - mean) / sqrt(var + eps) * w + b ; optional f32 copy y32.
void layernorm_launch(const float* x, const float* w, const float* b, void* y16, float* y32,
                      int64_t rows, int32_t dim, float eps, int32_t dtype, hipStream_t stream, const RowSegs* segs = nullptr);
// the same with the result quantised to MX fp8 (y8 [rows][dim] + block scales, activation layout)
void layernorm_fp8_launch(const float* x, const float* w, const float* b, uint8_t* y8, uint8_t* yscale, int64_t rows,
                          int32_t dim, float eps, hipStream_t stream, const RowSegs* segs = nullptr);
// u8 HWC -> f32 NCHW, reconstruction.rs:114-124
void preprocess_u8_launch(const uint8_t* rgb, float* img, int32_t batch, int32_t size,
                          hipStream_t stream);
// f32 NCHW -> f16 NCHW (same layout)
void cast_f32_to_16_launch(const float* src, void* dst, int64_t count, int32_t dtype,
                           hipStream_t stream);
void cast_16_to_f32_launch(const void* src, float* dst, int64_t count, int32_t dtype,
                           hipStream_t stream);
// bilinear resample of f32 planes [planes][in][in] -> 16-bit [planes][out][out] (encoder.rs:125-140)
void bilinear_launch(const float* src32, void* dst16, int32_t planes, int32_t in_size,
                     int32_t out_size, int32_t align_corners, int32_t dtype, hipStream_t stream);
// windows of the three pyramid levels -> patch matrix [(B*35)*g*g][3*256]; window order is
// image-major here: row = ((b*35 + win)*g*g + patch)
void patchify_launch(const void* x0, const void* x1, const void* x2, void* patches, int32_t batch,
                     int32_t grid, int32_t dtype, hipStream_t stream);
// one planar image stack [W][3][16g][16g] -> patch matrix [W*g*g][768]
void patchify_windows_launch(const void* xs16, void* patches, int32_t windows, int32_t grid,
                             int32_t dtype, hipStream_t stream);
// cls rows: tokens[w*(P+1)][:] = cls + pos[0]
void cls_rows_launch(float* tokens, const float* cls, const float* pos, int32_t windows,
                     int32_t tokens_per_window, int32_t dim, hipStream_t stream);
// encoder.rs:158-208 reshape_feature + merge: token rows of `steps*steps` windows (first window
// index win0 of each image's 35) -> NHWC f16 map [B][side][side][C], side = merged size.
// src is f32 tokens (src32) or f16 tokens (src16) with rows (b*35+win)*(P+1) + 1 + patch.
// split: dst16 holds [hi | lo] pairs of 2*dim channels per pixel (f32 source only)
void merge_launch(const float* src32, const void* src16, void* dst16, int32_t batch,
                  int32_t windows_per_image, int32_t win0, int32_t steps, int32_t padding,
                  int32_t grid, int32_t dim, int32_t dtype, hipStream_t stream, int32_t split = 0);
// NHWC (f16 or f32, optional zero border) <-> NCHW f32
void nhwc16_to_nchw32_launch(const void* src16, float* dst, int32_t batch, int32_t H, int32_t W,
                             int32_t C, int32_t border, int32_t dtype, hipStream_t stream, int32_t split = 0);
void nhwc32_to_nchw32_launch(const float* src, float* dst, int32_t batch, int32_t H, int32_t W,
                             int32_t C, hipStream_t stream);
// NCHW f32 -> NHWC: optional f32 copy, optional f16 copy (zero border, optional relu)
void nchw32_to_nhwc_launch(const float* src, float* dst32, void* dst16, int32_t batch, int32_t H,
                           int32_t W, int32_t C, int32_t border, int32_t relu16, int32_t dtype,
                           hipStream_t stream, int32_t split = 0);
// NHWC f32 -> 16-bit NHWC with a zero border (optional relu)
void nhwc32_to_16b_launch(const float* src, void* dst16b, int32_t batch, int32_t H, int32_t W,
                          int32_t C, int32_t relu, int32_t dtype, hipStream_t stream);
// channel concat of two NHWC f16 maps
void concat_channels_launch(const void* a, const void* b, void* dst, int64_t pixels, int32_t Ca,
                            int32_t Cb, hipStream_t stream);
// FOV tail (fov.rs:67-87)
void fov_add_relu_launch(const float* lin /*[B][P][C] tokens (cls dropped by caller offset)*/,
                         const float* low /*NHWC f32 [B][g][g][C]*/, void* dst16 /*bordered*/,
                         int32_t batch, int32_t grid, int32_t C, int32_t tokens_per_window,
                         int32_t dtype, hipStream_t stream);
void fov_final_launch(const void* x16 /*NHWC [B][k][k][C]*/, const float* w /*[k][k][C]*/,
                      const float* bias, float* fov_deg, float* f_norm, int32_t batch, int32_t k,
                      int32_t C, int32_t dtype, hipStream_t stream);

// ---------------------------------------------------------------------------------------
// Output back end (output.hip)
// ---------------------------------------------------------------------------------------
void depth_clamp_minmax_launch(float* depth, int64_t count, float* minmax_dev /*[2]*/,
                               hipStream_t stream);
// range_dev: device {min, max} (from depth_clamp_minmax_launch) used instead of the scalars when not null
// the sizes every stereogram entry accepts (ME_ERR_BAD_SHAPE otherwise); stereogram_launch starts with it
void stereogram_check_shape(int32_t rows, int32_t cols, int32_t out_w, int32_t out_h);
void stereogram_launch(const float* depth, int32_t rows, int32_t cols, float min_depth,
                       float max_depth, const float* range_dev, int32_t out_w, int32_t out_h, float amplitude,
                       const uint8_t* noise, uint8_t* out, hipStream_t stream);
void depthmap_rgb_launch(const float* depth, int64_t count, float min_depth, float max_depth,
                         const float* range_dev, uint8_t* rgb, hipStream_t stream);
// synchronises the stream (the counts come back to the host); workspace: mesh_workspace_bytes() device bytes
size_t mesh_workspace_bytes(int32_t width, int32_t height);
void mesh_index_run(const float* depth_dev, int32_t width, int32_t height, int32_t* vertex_index_dev,
                    int32_t* faces_dev /*nullable*/, int64_t* nverts, int64_t* nfaces, void* workspace,
                    hipStream_t stream);
void mesh_vertices_launch(const float* depth, int32_t width, int32_t height,
                          const int32_t* vertex_index, float xm, float ym, float* uv, float* xyz,
                          hipStream_t stream);
// OBJ text on the device (obj_format.hip): measure returns the exact size (header included), write fills the buffer
size_t obj_format_workspace_bytes(int64_t nverts, int64_t nfaces);
int64_t obj_format_measure(const float* uv, const float* xyz, const uint8_t* vertex_rgb, const int32_t* faces,
                           int64_t nverts, int64_t nfaces, bool tex, int64_t header_bytes, void* workspace,
                           hipStream_t stream);
void obj_format_write(const float* uv, const float* xyz, const uint8_t* vertex_rgb, const int32_t* faces, int64_t nverts,
                      int64_t nfaces, bool tex, char* text, void* workspace, hipStream_t stream);
void format_f64_launch(const double* v, int64_t n, char* out, int stride, int* lens, hipStream_t stream);
// the prefix sums of scan.h as the OBJ text (one workgroup) and the JPEG encoder (two levels, n > 0) run them
void obj_offsets_launch(const uint32_t* bytes, int64_t n, uint64_t base, uint64_t* off, hipStream_t stream);
void jpeg_encode_scan_offsets(me_ctx* ctx, const uint32_t* counts, int64_t n, uint64_t base, uint64_t* offsets);
void obj_vertex_colors_launch(const int32_t* vindex, const uint8_t* pixel_rgb, int64_t npix, uint8_t* vertex_rgb,
                              hipStream_t stream);
// Binary PLY records on the device (ply_format.hip): the vertex records (24 bytes, or 27 with vertex_rgb) and the face
// records (13 bytes) back to back from out + header_bytes; the size of the whole file, header included
int64_t ply_pack_bytes(int64_t nverts, bool with_rgb, int64_t nfaces, int64_t header_bytes);
void ply_pack_launch(const float* xyz, const uint8_t* vertex_rgb, int64_t nverts, const int32_t* faces, int64_t nfaces,
                     int64_t header_bytes, uint8_t* out, hipStream_t stream);
// glTF binary meshes on the device (glb_format.hip, layout in glb_format.h).  glb_bounds_run: the exact bounds of the
// written positions (x, -y, -z) of nverts > 0 vertices as sign keys (glb_format.h sign_key: three minima, three maxima),
// reduced in bounds_dev (24 bytes of device memory) and read back: it synchronises.  glb_pack_launch: every section of
// BIN (`second`: me_glb::Second, what stands between positions and indices), its gaps zeroed, from `bin` on, 16-byte aligned.
void glb_bounds_run(const float* xyz, int64_t nverts, int32_t* bounds_dev, int32_t keys[6], hipStream_t stream);
void glb_pack_launch(const float* xyz, const float* uv, const uint8_t* vertex_rgb, const int32_t* faces, int64_t nverts,
                     int64_t nfaces, int second, uint8_t* bin, hipStream_t stream);

}  // namespace me
