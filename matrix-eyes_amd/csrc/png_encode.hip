// PNG encoding on the device (RgbImage::save to ".png", output.rs:138 and :192): 8-bit RGB -> a complete PNG file in
// device memory.  Four launches, all on the context's stream (png_chunk.h holds the routines, DESIGN.md 4.28 the reasons):
//   png_filter_kernel   one workgroup per row: the five PNG filters, the cheapest kept -> the filtered stream [h][1 + 3w]
//   png_deflate_kernel  one workgroup per 64 KiB of that stream: LZ77 with an LDS head table (history primed from the
//                       preceding chunk's input), a dynamic Huffman block or stored blocks, ending byte-aligned (pigz's form)
//   png_layout_kernel   one workgroup: the prefix sum of the chunks' sizes, the Adler-32 from the chunks' partial sums,
//                       signature, IHDR, IEND
//   png_gather_kernel   one workgroup per chunk: its IDAT (one per deflate chunk) with the CRC-32, into the file
// The chunk kernels never wait for each other and use integer atomics only: the file is a pure function of the picture.
#include "model.h"
#include "png_chunk.h"

using namespace me;

namespace {

__global__ __launch_bounds__(me_png::kThreads) void png_filter_kernel(const uint8_t* rgb, int32_t w, uint8_t* stream) {
    __shared__ me_png::FilterShared S;
    me_png::filter_row(S, rgb, w, (int32_t)blockIdx.x, stream);
}

__global__ __launch_bounds__(me_png::kThreads) void png_deflate_kernel(const uint8_t* stream, int64_t total, int64_t stride, int64_t nchunks,
                                                                       uint32_t* syms, uint8_t* slots,
                                                                       me_png::ChunkInfo* info) {
    __shared__ me_png::ChunkShared S;
    const int64_t c = blockIdx.x;
    me_png::deflate_chunk(S, stream, total, stride, c, nchunks, syms + c * me_png::kChunk, slots + c * me_png::kSlot, info + c);
}

__global__ __launch_bounds__(me_png::kThreads) void png_layout_kernel(const me_png::ChunkInfo* info, int64_t nchunks, int32_t w,
                                                                      int32_t h, uint8_t* file, int64_t* offsets, int64_t* meta) {
    me_png::layout_file(info, nchunks, w, h, file, offsets, meta);
}

__global__ __launch_bounds__(me_png::kThreads) void png_gather_kernel(const me_png::ChunkInfo* info, const uint8_t* slots,
                                                                      int64_t nchunks, const int64_t* offsets, const int64_t* meta,
                                                                      uint8_t* file) {
    __shared__ me_png::GatherShared S;
    const int64_t c = blockIdx.x;
    me_png::gather_idat(S, info, slots + c * me_png::kSlot, c, nchunks, offsets, meta, file);
}

}  // namespace

namespace me {

void check_png_shape(const char* who, int32_t w, int32_t h) {
    ME_CHECK(w > 0 && h > 0, ME_ERR_BAD_SHAPE, "%s: %dx%d", who, w, h);
    ME_CHECK(w <= ME_RESIZE_MAX_DIM && h <= ME_RESIZE_MAX_DIM, ME_ERR_BAD_SHAPE,
             "%s: %dx%d: a side exceeds ME_RESIZE_MAX_DIM (%d)", who, w, h, ME_RESIZE_MAX_DIM);
}

// rgb [h,w,3] in device memory -> the file in the context's scratch; synchronises (the size comes back to the host)
DeviceFile png_encode_device(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h) {
    using namespace me_png;
    hipStream_t s = ctx->stream;
    // the output back end may run on its own stream (me_ctx_set_output_overlap): its scratch is its own
    const std::string tag = (ctx->out_stream && s == ctx->out_stream) ? "out.png." : "png.";
    const int64_t total = ((int64_t)w * 3 + 1) * h, nchunks = (total + kChunk - 1) / kChunk;
    uint8_t* stream = (uint8_t*)site_buf(ctx, tag + "stream", (size_t)total);
    uint32_t* syms = (uint32_t*)site_buf(ctx, tag + "syms", (size_t)nchunks * kChunk * sizeof(uint32_t));
    uint8_t* slots = (uint8_t*)site_buf(ctx, tag + "slots", (size_t)nchunks * kSlot);
    ChunkInfo* info = (ChunkInfo*)site_buf(ctx, tag + "info", (size_t)nchunks * sizeof(ChunkInfo));
    int64_t* offsets = (int64_t*)site_buf(ctx, tag + "offsets", (size_t)(nchunks + 3) * sizeof(int64_t));
    int64_t* meta = offsets + nchunks;
    const size_t capacity = (size_t)kFileSlack + (size_t)nchunks * (kSlot + 12);
    uint8_t* file = (uint8_t*)site_buf(ctx, tag + "file", capacity);

    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)h), dim3(kThreads), 0, s, rgb, w, stream);
    ME_HIP(hipGetLastError());
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, stream, total, (int64_t)w * 3 + 1, nchunks, syms, slots, info);
    ME_HIP(hipGetLastError());
    hipLaunchKernelGGL(png_layout_kernel, dim3(1), dim3(kThreads), 0, s, info, nchunks, w, h, file, offsets, meta);
    ME_HIP(hipGetLastError());
    hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, info, slots, nchunks, offsets, meta, file);
    ME_HIP(hipGetLastError());
    int64_t host_meta[3] = {0, 0, 0};
    ME_HIP(hipMemcpyAsync(host_meta, meta, sizeof(host_meta), hipMemcpyDeviceToHost, s));
    ME_HIP(hipStreamSynchronize(s));
    ME_CHECK(host_meta[0] > 0 && (size_t)host_meta[0] <= capacity && !(host_meta[2] & 2), ME_ERR_HIP,
             "png: a chunk's packed size differs from its estimate (file %lld bytes, flags %lld)", (long long)host_meta[0],
             (long long)host_meta[2]);
    DeviceFile f;
    f.dev = file, f.bytes = host_meta[0];
    return f;
}

}  // namespace me
