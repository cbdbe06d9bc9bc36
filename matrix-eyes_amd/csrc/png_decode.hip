// PNG decoding on the GPU (reconstruction.rs:95-113 for the photo, output.rs:206-218 for the vertex colours:
// ImageReader::open(..).decode().into_rgb8() + apply_orientation), byte for byte what the C++ host layer's decoder
// (host/png_decoder.cpp decode_png) followed by apply_orientation (host/image_io.cpp) writes.
//
// The host keeps zlib's inflate (one chain of back-references) and lets it land in pinned memory; everything behind it runs
// here, on the context's stream, band by band while the host is still inflating:
//   png_unfilter_kernel  the filtered stream -> the reconstructed stream (same layout: filter byte + row, pass after pass),
//                        a skewed wavefront: a wave owns 64 consecutive rows, one per lane; at step t lane l reconstructs
//                        pixel t - l, takes b from the lane above by a cross-lane move of what that lane made one step
//                        earlier, c is its own b of the step before, a its own result of the step before
//   png_finish_kernel    the reconstructed stream -> oriented RGB: every colour type and depth, de-interlacing and the
//                        orientation as a remap of the store address, one pass over the picture's pixels
// The arithmetic is png_recon.h's, shared with the host decoder and the host driver of the CPU tests.  Integer kernels on
// the HBM side, no MFMA.
//
// Dependencies: rows of one pass depend on the row above.  Inside a workgroup the row groups of a pass trail each other by
// one tile (barriers between the tile steps); between workgroups the only dependency is the launch order on the stream: a
// band of rows is one launch, and no workgroup ever waits for another.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "../host/image_io.hpp"
#include "model.h"
#include "png_recon.h"

namespace me {

namespace {

using namespace me_pngdec;

constexpr int kWaves = 4;             // row groups of one pass in flight in a workgroup, each one tile behind the one above
constexpr int kGroupRows = 64;        // rows of a group: one per lane
// Bytes of a row in one LDS tile: a multiple of every bpp (1, 2, 3, 4, 6, 8).  A tile row is kTileBytes + BPP + 4 bytes
// apart from the next, so that lane l's byte at step t, l * (pitch - BPP) + t * BPP, moves 55 dwords (odd) from lane to
// lane: the 32 lanes of a ds_read_u8 / ds_write_b8 group fall into 32 different banks.
constexpr int kTileBytes = 216;
constexpr int kLoadRows = 16;                             // rows of a tile a wave has in flight while it stages the tile
constexpr int kLoadCols = (kTileBytes + 63) / 64;         // bytes of a tile row per lane
constexpr int kDefaultBandRows = kWaves * kGroupRows;
constexpr int kMaxBands = 64;         // the default band grows with the picture: at most this many launches
constexpr int kFinishMaxGrid = 1024;  // 4 workgroups on each of 256 CUs; more pixels than this covers: further grid rounds

struct Band {
    int32_t py0[kMaxPasses], py1[kMaxPasses];   // rows of each pass in this launch
};

// One workgroup per pass.  Wave w takes row groups w, w + kWaves, ... of the band's rows of its pass; within a round of
// kWaves groups, wave w works on tile s - w at tile step s, so the last row of the group above is finished (and in dst:
// the barrier at the end of a tile step orders the stores of the workgroup) when its first lane needs it.  src == dst:
// in place.
template <int BPP>
__global__ __launch_bounds__(kWaves * 64) void png_unfilter_kernel(const Geom g, const Band band, const uint8_t* src,
                                                                   uint8_t* dst) {
    constexpr int kPitch = kTileBytes + BPP + 4;
    __shared__ uint8_t tiles[kWaves][(kGroupRows + 1) * kPitch];   // row 0: the row above the group
    const int ps = (int)blockIdx.x;
    const Pass p = g.pass[ps];
    const int r0 = band.py0[ps], r1 = band.py1[ps];
    if (r0 >= r1) return;   // the whole workgroup
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t row_pitch = (int64_t)p.stride + 1;
    const int ngroups = (r1 - r0 + kGroupRows - 1) / kGroupRows;
    const int ntiles = (p.stride + kTileBytes - 1) / kTileBytes;
    uint8_t* const tile = tiles[wave];
    uint8_t* const my_row = tile + (lane + 1) * kPitch;

    for (int round = 0; round * kWaves < ngroups; ++round) {
        const int group = round * kWaves + wave;
        const int row0 = r0 + group * kGroupRows;
        const int nrows = group < ngroups ? min(kGroupRows, r1 - row0) : 0;
        int filter = 0;
        LaneState<BPP> st;
        lane_reset(st);
        if (lane < nrows) {
            const int64_t at = p.offset + (int64_t)(row0 + lane) * row_pitch;
            filter = src[at];
            if (dst != src) dst[at] = (uint8_t)filter;
            if (filter > 4) filter = 0;   // the host refuses such a stream before it gets here
        }
        for (int s = 0; s < ntiles + kWaves - 1; ++s) {
            const int k = s - wave;
            const bool work = nrows > 0 && k >= 0 && k < ntiles;   // the same for every lane of a wave
            const int xb = k * kTileBytes;
            const int tb = work ? min(kTileBytes, p.stride - xb) : 0;
            const int npx = tb / BPP;
            // rows in, in coalesced segments
            if (work) {
                const int64_t above = p.offset + (int64_t)(row0 - 1) * row_pitch + 1 + xb;
                for (int c = lane; c < tb; c += 64) tile[c] = row0 > 0 ? dst[above + c] : (uint8_t)0;
                // kLoadRows rows at a time: their loads are all in flight before the first one is waited for
                for (int r = 0; r < nrows; r += kLoadRows) {
                    uint8_t v[kLoadRows][kLoadCols];
#pragma unroll
                    for (int j = 0; j < kLoadRows; ++j) {
                        const int64_t at = p.offset + (int64_t)(row0 + r + j) * row_pitch + 1 + xb;
#pragma unroll
                        for (int q = 0; q < kLoadCols; ++q) {
                            const int c = lane + 64 * q;
                            v[j][q] = r + j < nrows && c < tb ? src[at + c] : (uint8_t)0;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < kLoadRows; ++j)
#pragma unroll
                        for (int q = 0; q < kLoadCols; ++q) {
                            const int c = lane + 64 * q;
                            if (r + j < nrows && c < tb) tile[(r + j + 1) * kPitch + c] = v[j][q];
                        }
                }
            }
            __syncthreads();
            // the diagonal: every lane shifts its last result to the lane below, then the lanes inside the tile step
            if (work) {
                for (int t = 0; t < npx + nrows - 1; ++t) {
                    uint32_t lo = 0, hi = 0;
#pragma unroll
                    for (int i = 0; i < BPP; ++i) {
                        if (i < 4) lo |= (uint32_t)st.a[i] << (8 * i);
                        else hi |= (uint32_t)st.a[i] << (8 * (i - 4));
                    }
                    lo = __shfl_up(lo, 1);
                    if (BPP > 4) hi = __shfl_up(hi, 1);
                    const int px = t - lane;
                    if (lane < nrows && px >= 0 && px < npx) {
                        uint8_t above[BPP], x[BPP];
#pragma unroll
                        for (int i = 0; i < BPP; ++i) {
                            above[i] = lane == 0 ? tile[px * BPP + i] : (uint8_t)((i < 4 ? lo >> (8 * i) : hi >> (8 * (i - 4))) & 0xff);
                            x[i] = my_row[px * BPP + i];
                        }
                        lane_step<BPP>(st, filter, above, x);
#pragma unroll
                        for (int i = 0; i < BPP; ++i) my_row[px * BPP + i] = x[i];
                    }
                }
            }
            __syncthreads();
            // rows out
            if (work) {
                for (int r = 0; r < nrows; ++r) {
                    const int64_t at = p.offset + (int64_t)(row0 + r) * row_pitch + 1 + xb;
                    for (int c = lane; c < tb; c += 64) dst[at + c] = tile[(r + 1) * kPitch + c];
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

// One lane: one pixel of the decoded picture per grid round, in picture order, so that for orientations 1..4 the lanes of a
// wave store a contiguous run of the destination row (2 and 3 reversed); 5..8 turn the run into a column.
__global__ __launch_bounds__(256) void png_finish_kernel(const Geom g, const int32_t orientation,
                                                         const uint8_t* __restrict__ stream, const uint8_t* __restrict__ plte,
                                                         const int32_t plte_bytes, uint8_t* __restrict__ dst,
                                                         int32_t* __restrict__ status) {
    __shared__ Pass passes[kMaxPasses];
    if (threadIdx.x < kMaxPasses) passes[threadIdx.x] = g.pass[threadIdx.x];
    __syncthreads();
    const int64_t n = (int64_t)g.width * g.height;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t y = (int32_t)(i / g.width), x = (int32_t)(i - (int64_t)y * g.width);
        int32_t px, py;
        const Pass& p = passes[pass_pixel(g, x, y, &px, &py)];
        const uint8_t* row = stream + p.offset + (int64_t)py * ((int64_t)p.stride + 1) + 1;
        uint8_t rgb[3] = {0, 0, 0};
        if (!pixel_rgb(g, row, px, plte, plte_bytes, rgb)) atomicOr(status, 1);
        uint8_t* o = dst + dest_index(g, p, px, py, orientation) * 3;
        o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
    }
}

template <int BPP>
void launch_unfilter(const Geom& g, const Band& band, const uint8_t* src, uint8_t* dst, hipStream_t s) {
    hipLaunchKernelGGL(png_unfilter_kernel<BPP>, dim3((unsigned)g.npass), dim3(kWaves * 64), 0, s, g, band, src, dst);
}

// every band of the picture whose rows are complete at `complete` stream bytes and not yet launched
struct Unfilter {
    Geom g;
    int32_t band_rows = kDefaultBandRows;
    int32_t nbands = 0, next = 0;
    hipStream_t stream = nullptr;

    void plan(const Geom& geom, int32_t rows) {
        g = geom;
        band_rows = rows > 0 ? rows : std::max<int64_t>(kDefaultBandRows, cdiv(cdiv(g.height, kMaxBands), kDefaultBandRows) * kDefaultBandRows);
        nbands = (int32_t)cdiv(g.height, band_rows), next = 0;
    }
    Band band(int32_t i) const {
        Band b;
        for (int ps = 0; ps < kMaxPasses; ++ps)
            band_rows_of(g.pass[ps], (int64_t)i * band_rows, std::min<int64_t>(g.height, ((int64_t)i + 1) * band_rows), &b.py0[ps], &b.py1[ps]);
        return b;
    }
    // the stream bytes band b needs complete
    int64_t end_of(const Band& b) const {
        int64_t end = 0;
        for (int ps = 0; ps < g.npass; ++ps)
            if (b.py1[ps] > b.py0[ps]) end = std::max(end, g.pass[ps].offset + (int64_t)b.py1[ps] * ((int64_t)g.pass[ps].stride + 1));
        return end;
    }
    void launch(const Band& b, const uint8_t* src, uint8_t* dst) const {
        bool any = false;
        for (int ps = 0; ps < g.npass; ++ps) any = any || b.py1[ps] > b.py0[ps];
        if (!any) return;
        switch (g.bpp) {
            case 1: launch_unfilter<1>(g, b, src, dst, stream); break;
            case 2: launch_unfilter<2>(g, b, src, dst, stream); break;
            case 3: launch_unfilter<3>(g, b, src, dst, stream); break;
            case 4: launch_unfilter<4>(g, b, src, dst, stream); break;
            case 6: launch_unfilter<6>(g, b, src, dst, stream); break;
            case 8: launch_unfilter<8>(g, b, src, dst, stream); break;
            default: fail(ME_ERR_BAD_ARG, "PNG unfilter: %d bytes per pixel", g.bpp);
        }
        ME_HIP(hipGetLastError());
    }
};

// a filter byte above 4 among the band's rows (the host scans them as the band completes: ph bytes per pass)
bool bad_filter(const Geom& g, const Band& b, const uint8_t* stream) {
    for (int ps = 0; ps < g.npass; ++ps) {
        const Pass& p = g.pass[ps];
        for (int32_t py = b.py0[ps]; py < b.py1[ps]; ++py)
            if (stream[p.offset + (int64_t)py * ((int64_t)p.stride + 1)] > 4) return true;
    }
    return false;
}

// what inflate_png's callback works with: bands are uploaded and launched as the inflate completes them
struct Feed {
    me_ctx* ctx;
    Unfilter u;
    const uint8_t* pinned;
    uint8_t* dev;
    int64_t uploaded = 0;
    bool defect = false;

    void upto(size_t complete) {
        while (!defect && u.next < u.nbands) {
            const Band b = u.band(u.next);
            const int64_t end = u.end_of(b);
            if (end > (int64_t)complete) break;
            if (bad_filter(u.g, b, pinned)) {
                defect = true;
                break;
            }
            hipStream_t s = u.stream;
            ctx->png_marks.record(3 * (size_t)u.next, s);
            if (end > uploaded) {
                ME_HIP(hipMemcpyAsync(dev + uploaded, pinned + uploaded, (size_t)(end - uploaded), hipMemcpyHostToDevice, s));
                uploaded = end;
            }
            ctx->png_marks.record(3 * (size_t)u.next + 1, s);
            u.launch(b, dev, dev);
            ctx->png_marks.record(3 * (size_t)u.next + 2, s);
            ++u.next;
        }
    }
    static void callback(void* user, size_t complete) { ((Feed*)user)->upto(complete); }
};

// the pinned buffer the inflate lands in (the upload of the call before may still be reading it), and the status word
uint8_t* pinned_stream(me_ctx* ctx, size_t bytes) {
    if (!ctx->png_status) ME_HIP(hipHostMalloc((void**)&ctx->png_status, sizeof(int32_t), hipHostMallocDefault));
    return (uint8_t*)ctx->png_upload.reserve(bytes);
}

// The device path met a defect (the stream does not inflate, a filter byte above 4, a palette index past the palette): the
// host decoder runs whole and meets the file's defects in stream order; its ImageError is the answer.
[[noreturn]] void refuse_as_the_host(const std::vector<uint8_t>& bytes, const std::string& name) {
    try {
        (void)matrix_eyes::decode_png(bytes, name, nullptr);
    } catch (const matrix_eyes::ImageError& err) {
        fail(ME_ERR_BAD_ARG, "%s", err.what());
    }
    fail(ME_ERR_HIP, "%s: the device PNG decoder refused a file the host decoder accepts", name.c_str());
}

}  // namespace

void free_png_scratch(me_ctx* ctx) {
    ctx->png_upload.release();
    if (ctx->png_status) (void)hipHostFree(ctx->png_status);
    ctx->png_status = nullptr;
    ctx->png_marks.destroy();
}

uint8_t* png_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst_dev,
                         int32_t want_w, int32_t want_h, int32_t* ow, int32_t* oh) {
    const std::string name = "<png>";
    const std::vector<uint8_t> bytes(file, file + nbytes);
    hipStream_t s = ctx->stream;
    ctx->png_timed = false;
    matrix_eyes::PngFrame f;
    try {
        f = matrix_eyes::parse_png_header(bytes, name);
    } catch (const matrix_eyes::ImageError& err) {
        fail(ME_ERR_BAD_ARG, "%s", err.what());
    }
    // the size first: a caller's buffer of another size is refused before any decoding
    oriented_size_or_refuse("PNG", (int32_t)f.width, (int32_t)f.height, orientation, want_w, want_h, ow, oh);

    uint8_t* pinned = pinned_stream(ctx, f.total);
    uint8_t* stream = (uint8_t*)site_buf(ctx, "png.stream", f.total);
    uint8_t* plte = (uint8_t*)site_buf(ctx, "png.plte", 768);
    int32_t* status = (int32_t*)site_buf(ctx, "png.status", sizeof(int32_t));
    if (!dst_dev) dst_dev = (uint8_t*)site_buf(ctx, "png.rgb", (size_t)f.width * f.height * 3);

    Feed feed{ctx, Unfilter(), pinned, stream};
    feed.u.plan(f.geom, 0);
    feed.u.stream = s;
    bool inflated = true;
    const auto t0 = std::chrono::steady_clock::now();
    try {
        matrix_eyes::inflate_png(f, bytes, name, pinned, Feed::callback, &feed);
    } catch (const matrix_eyes::ImageError&) {
        inflated = false;
    }
    ctx->png_inflate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (feed.uploaded > 0) ctx->png_upload.uploaded_on(s);
    if (!inflated || feed.defect || feed.u.next != feed.u.nbands) refuse_as_the_host(bytes, name);
    const size_t band_events = 3 * (size_t)feed.u.nbands;

    const bool palette = f.ctype == 3;
    const size_t plte_bytes = std::min<size_t>(f.plte.size(), 768);   // an index reaches 255: 3 * 255 + 2 < 768
    if (palette) {
        // pageable memory: the copy has left f.plte when the call returns
        if (plte_bytes) ME_HIP(hipMemcpyAsync(plte, f.plte.data(), plte_bytes, hipMemcpyHostToDevice, s));
        ME_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    }
    ctx->png_marks.record(band_events, s);
    const int64_t pixels = (int64_t)f.width * f.height;
    hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)std::min<int64_t>(cdiv(pixels, 256), kFinishMaxGrid)), dim3(256), 0, s,
                       f.geom, orientation, (const uint8_t*)stream, (const uint8_t*)plte, (int32_t)plte_bytes, dst_dev, status);
    ME_HIP(hipGetLastError());
    ctx->png_marks.record(band_events + 1, s);
    if (palette) {   // the one case that waits for the device: the status word decides between pixels and a refusal
        ME_HIP(hipMemcpyAsync(ctx->png_status, status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ME_HIP(hipStreamSynchronize(s));
        if (*ctx->png_status) refuse_as_the_host(bytes, name);
    }
    ctx->png_timed = true, ctx->png_timed_download = false, ctx->png_timed_bands = feed.u.nbands;
    return dst_dev;
}

void png_unfilter(me_ctx* ctx, const uint8_t* src_dev, uint8_t* dst_dev, int32_t width, int32_t height, int32_t depth,
                  int32_t ctype, int32_t interlace, int32_t band_rows) {
    Unfilter u;
    u.plan(make_geom(width, height, depth, ctype, interlace), band_rows);
    u.stream = ctx->stream;
    for (int32_t i = 0; i < u.nbands; ++i) u.launch(u.band(i), src_dev, dst_dev);
}

}  // namespace me
