// JPEG decoding on the GPU (reconstruction.rs:95-106: ImageReader::open(..).decode() + apply_orientation), byte for byte
// what the C++ host layer's decoder (host/jpeg_decoder.cpp) followed by apply_orientation (host/image_io.cpp) writes.
//
// The entropy-coded segments are decoded on the host (decode_jpeg_coefficients: the serial part, every scan type) straight
// into pinned memory; the coefficients go up on the context's stream and two kernels reconstruct the picture:
//   jpeg_idct_kernel    coefficients + quantisation tables -> the components' u8 planes (one wave per 8x8 block: dequantise,
//                       the DC-only vote, row pass, column pass through LDS, level shift, clamp)
//   jpeg_finish_kernel  planes -> oriented RGB: chroma upsampling, colour conversion and the orientation as a remap of the
//                       store address, one pass over the output pixels
// With me_ctx_set_jpeg_entropy(ctx, 1) the scan's bytes go up instead and the coefficients are made on the device
// (jpeg_entropy.hip); a file that decoder declines takes the host path above, whole.
// The arithmetic is jpeg_recon.h's, shared with the host driver of the CPU tests; this unit is compiled with contraction off
// (pragma below and the Makefile rule) as resample.hip is: a fused multiply-add in the IDCT changes bytes.  The IDCT basis
// comes from the one host function both decoders use (jpeg_basis.cpp) -- no device cos.  HBM-side kernels, no MFMA.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "../host/image_io.hpp"
#include "jpeg_recon.h"
#include "model.h"

#pragma clang fp contract(off)

namespace me {

namespace {

using namespace me_jpeg;

constexpr int kIdctWaves = 4;            // waves of a workgroup = blocks it has in flight
constexpr int kIdctBlocksPerWave = 8;    // blocks a wave takes of one chunk, one after the other
constexpr int kIdctChunk = kIdctWaves * kIdctBlocksPerWave;   // 32 neighbouring blocks per workgroup and grid round
constexpr int kIdctMaxGrid = 1024;       // 4 workgroups on each of 256 CUs; more chunks than this: further grid rounds
constexpr int kFinishPixels = 4;         // horizontally adjacent pixels of one lane of the finish kernel

__device__ __forceinline__ CompDesc pick_comp(const Frame& f, int ci) {
    return ci == 0 ? f.comp[0] : (ci == 1 ? f.comp[1] : f.comp[2]);  // selects, not an indexed copy of the argument
}

// Blocks of all components are numbered one component after the other; chunk k is blocks [32 k, 32 k + 32): wave w takes
// blocks 32 k + 4 i + w for i = 0..7, so the four waves read 512 contiguous bytes of coefficients per step.  The barrier
// count is the same for every wave (an inactive block only keeps the barriers company).  Padded blocks of the planes are
// written like any other (the host's planes hold them too); jpeg_finish_kernel never reads them as samples.
__global__ __launch_bounds__(kIdctWaves * 64) void jpeg_idct_kernel(const Frame f, const IdctTables tab,
                                                                     const int16_t* __restrict__ coef,
                                                                     uint8_t* __restrict__ planes) {
    __shared__ BlockShared sh[kIdctWaves];
    __shared__ double basis[64];
    __shared__ uint16_t q[kMaxComps][64];
    const int tid = (int)threadIdx.x;
    if (tid < 64) basis[tid] = tab.basis[tid];
    if (tid < kMaxComps * 64) q[tid >> 6][tid & 63] = tab.q[tid >> 6][tid & 63];
    __syncthreads();
    const int wave = tid >> 6;
    const int nchunks = (f.total_blocks + kIdctChunk - 1) / kIdctChunk;
    for (int chunk = (int)blockIdx.x; chunk < nchunks; chunk += (int)gridDim.x) {
        for (int i = 0; i < kIdctBlocksPerWave; ++i) {
            const int blk = chunk * kIdctChunk + i * kIdctWaves + wave;
            const bool active = blk < f.total_blocks;
            int ci = 0;
            if (f.ncomp == 3) ci = blk >= f.comp[2].block0 ? 2 : (blk >= f.comp[1].block0 ? 1 : 0);
            const CompDesc c = pick_comp(f, ci);
            const int lb = active ? blk - c.block0 : 0;
            const int by = lb / c.blocks_w, bx = lb - by * c.blocks_w;
            idct_block(sh[wave], active, coef + c.coef_off + (int64_t)lb * 64, q[ci], basis,
                       planes + c.plane_off + (int64_t)by * 8 * c.pw + (int64_t)bx * 8, c.pw);
        }
    }
}

// One lane: kFinishPixels neighbouring pixels of one row of the decoded picture (their chroma samples are the same few
// bytes).  Orientations 1..4 keep the run contiguous in the output (2 and 3 reversed): its 12 bytes leave as three dwords
// when they start on a dword boundary; orientations 5..8 turn the run into a column, one pixel per row.
__global__ __launch_bounds__(256) void jpeg_finish_kernel(const Frame f, const uint8_t* __restrict__ planes,
                                                          uint8_t* __restrict__ dst) {
    const int x0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * kFinishPixels;
    const int y = (int)blockIdx.y;
    if (x0 >= f.width) return;
    const int n = min(kFinishPixels, f.width - x0);
    uint8_t px[kFinishPixels * 3];
#pragma unroll
    for (int k = 0; k < kFinishPixels; ++k)
        if (k < n) pixel_rgb(f, planes, x0 + k, y, &px[3 * k]);
    if (f.orientation <= 4) {
        const bool reversed = f.orientation == 2 || f.orientation == 3;
        uint8_t* p = dst + oriented_index(f, reversed ? x0 + n - 1 : x0, y) * 3;
        if (n == kFinishPixels && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            uint32_t w[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < kFinishPixels; ++k) {
                const int s = reversed ? kFinishPixels - 1 - k : k;   // source pixel of output slot k
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int at = 3 * k + c;
                    w[at >> 2] |= (uint32_t)px[3 * s + c] << (8 * (at & 3));
                }
            }
            uint32_t* p4 = reinterpret_cast<uint32_t*>(p);
            p4[0] = w[0], p4[1] = w[1], p4[2] = w[2];
        } else {
            for (int k = 0; k < n; ++k) {
                const int s = reversed ? n - 1 - k : k;
                p[3 * k] = px[3 * s], p[3 * k + 1] = px[3 * s + 1], p[3 * k + 2] = px[3 * s + 2];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < kFinishPixels; ++k)
            if (k < n) {
                uint8_t* p = dst + oriented_index(f, x0 + k, y) * 3;
                p[0] = px[3 * k], p[1] = px[3 * k + 1], p[2] = px[3 * k + 2];
            }
    }
}

// pinned memory for the entropy decoder (JpegCoefAlloc): the upload of the call before may still be reading the buffer
int16_t* pinned_coefficients(void* user, size_t count) { return jpeg_pinned_buffer((me_ctx*)user, count); }

// frame geometry, upsampling modes and colour handling of Decoder::finish, and the tables of Decoder::idct_all
void plan(const matrix_eyes::JpegCoefficients& c, int32_t orientation, Frame& f, IdctTables& tab, size_t& plane_bytes) {
    std::memset(&f, 0, sizeof(f));
    std::memset(&tab, 0, sizeof(tab));
    f.width = c.width, f.height = c.height, f.ncomp = (int32_t)c.comps.size(), f.orientation = orientation;
    int64_t coef_off = 0, plane_off = 0;
    int32_t block0 = 0;
    for (int i = 0; i < f.ncomp; ++i) {
        const matrix_eyes::JpegComponent& k = c.comps[(size_t)i];
        CompDesc& d = f.comp[i];
        d.width = k.width, d.height = k.height, d.blocks_w = k.blocks_w, d.blocks_h = k.blocks_h, d.pw = k.blocks_w * 8;
        d.fx = c.hmax / k.h, d.fy = c.vmax / k.v;
        const int n = k.width;
        d.mode = d.fx == 1 && d.fy == 1 ? UP_COPY
                 : d.fx == 2 && d.fy == 1 && n > 2 ? UP_H2V1
                 : d.fx == 2 && d.fy == 2 && n > 2 ? UP_H2V2
                 : d.fx == 1 && d.fy == 2 ? UP_H1V2 : UP_REPL;
        d.block0 = block0, d.qsel = i, d.coef_off = coef_off, d.plane_off = plane_off;
        const int64_t blocks = (int64_t)k.blocks_w * k.blocks_h;
        block0 += (int32_t)blocks, coef_off += blocks * 64, plane_off += blocks * 64;
        for (int j = 0; j < 64; ++j) tab.q[i][j] = c.qt[k.tq][j];
    }
    f.total_blocks = block0;
    plane_bytes = (size_t)plane_off;
    const bool rgb = f.ncomp == 3 && (c.adobe_transform == 0 || (c.adobe_transform < 0 && c.comps[0].id == 'R' &&
                                                                 c.comps[1].id == 'G' && c.comps[2].id == 'B'));
    f.color = f.ncomp == 1 ? COLOR_GREY : (rgb ? COLOR_RGB : COLOR_YCC);
    matrix_eyes::jpeg_idct_basis(tab.basis);
}

}  // namespace

void free_jpeg_scratch(me_ctx* ctx) {
    free_jpeg_entropy_scratch(ctx);
    free_jpeg_encode_scratch(ctx);
    ctx->jpeg_upload.release();
    ctx->jpeg_marks.destroy();
}

uint8_t* jpeg_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst_dev,
                          int32_t want_w, int32_t want_h, int32_t* ow, int32_t* oh) {
    const std::string name = "<jpeg>";
    const std::vector<uint8_t> bytes(file, file + nbytes);
    hipStream_t s = ctx->stream;
    ctx->jpeg_timed = false;
    matrix_eyes::JpegCoefficients c;
    bool on_device = false;  // the coefficients are in "jpeg.coef" already (jpeg_entropy.hip)
    try {
        // the size first: a caller's buffer of another size is refused before any decoding
        const matrix_eyes::JpegCoefficients head = matrix_eyes::parse_jpeg_header(bytes, name);
        oriented_size_or_refuse("JPEG", head.width, head.height, orientation, want_w, want_h, ow, oh);
        const auto t0 = std::chrono::steady_clock::now();
        ctx->jpeg_entropy_reported = false;
        if (ctx->jpeg_entropy_mode == 1) {
            // a decline judges nothing: the host decoder below runs whole, and its pixels or its words stand
            matrix_eyes::JpegEntropyPlan entropy;
            on_device = jpeg_entropy_decode(ctx, bytes, 0, entropy);
            if (on_device) c = std::move(entropy.frame);
        }
        if (!on_device) c = matrix_eyes::decode_jpeg_coefficients(bytes, name, pinned_coefficients, ctx);
        ctx->jpeg_entropy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        matrix_eyes::check_jpeg_reconstructible(c, name);
    } catch (const matrix_eyes::ImageError& err) {
        fail(ME_ERR_BAD_ARG, "%s", err.what());
    }
    Frame f;
    IdctTables tab;
    size_t plane_bytes = 0;
    plan(c, orientation, f, tab, plane_bytes);

    int16_t* coef = (int16_t*)site_buf(ctx, "jpeg.coef", c.total_coefs * sizeof(int16_t));
    uint8_t* planes = (uint8_t*)site_buf(ctx, "jpeg.planes", plane_bytes);
    if (!dst_dev) dst_dev = (uint8_t*)site_buf(ctx, "jpeg.rgb", (size_t)f.width * f.height * 3);

    ctx->jpeg_marks.record(0, s);
    if (!on_device) {
        ME_HIP(hipMemcpyAsync(coef, c.comps[0].coef, c.total_coefs * sizeof(int16_t), hipMemcpyHostToDevice, s));
        ctx->jpeg_upload.uploaded_on(s);
    }
    ctx->jpeg_marks.record(1, s);

    const int nchunks = (int)cdiv(f.total_blocks, kIdctChunk);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)std::min(nchunks, kIdctMaxGrid)), dim3(kIdctWaves * 64), 0, s, f, tab,
                       (const int16_t*)coef, planes);
    ME_HIP(hipGetLastError());
    ctx->jpeg_marks.record(2, s);

    const dim3 fgrid((unsigned)cdiv(cdiv(f.width, kFinishPixels), 256), (unsigned)f.height);
    hipLaunchKernelGGL(jpeg_finish_kernel, fgrid, dim3(256), 0, s, f, (const uint8_t*)planes, dst_dev);
    ME_HIP(hipGetLastError());
    ctx->jpeg_marks.record(3, s);
    ctx->jpeg_timed = true, ctx->jpeg_timed_download = false;
    return dst_dev;
}

}  // namespace me
