// Baseline JPEG encoding on the device (RgbImage::save to ".jpg" / ".jpeg", output.rs:138 and :192): 8-bit RGB -> a complete
// JFIF file in device memory, byte for byte the file libjpeg writes (csrc/jpeg_encode.h holds the routines and the rules,
// DESIGN.md 4.31 the reasons).  All launches are on the context's stream:
//   jpeg_fdct_kernel          8 lanes per block, 32 blocks per workgroup, blocks in scan order: samples gathered from the RGB
//                             picture, row pass, transpose through LDS, column pass, quantisation -> int16 zigzag coefficients
//   jpeg_bits_kernel          one wave per block, lane k = zigzag position k: the block's bit count
//   scan_groups_kernel        exclusive sums inside a workgroup and the workgroup's aggregate, 64-bit (scan.h) ...
//   scan_slices_kernel        ... and one workgroup over the aggregates; both are used twice (block bits, stuffed bytes)
//   jpeg_pack_kernel          the codes again, ORed into the zeroed big-endian stream at their bit offsets (vector atomic OR:
//                             OR commutes, so the bytes do not depend on the order); the last lane pads with ones
//   jpeg_stuff_count_kernel   FF bytes per 16 bytes of the packed stream
//   jpeg_stuff_kernel         the scatter behind the header with 00 behind each FF; the header and FFD9
// No kernel waits for another workgroup: workgroups meet at launch boundaries only.  Every loop is bounded by a block's 64
// coefficients, a lane's 16 bytes, or a workgroup's share of the aggregates.  The host reads back two numbers: the scan's
// bits (the packed stream is sized from them) and the file's size.
#include <cstring>
#include <vector>

#include "jpeg_encode.h"
#include "model.h"
#include "scan.h"

using namespace me;

namespace {

using namespace me_jpeg_encode;

__global__ __launch_bounds__(kThreads) void jpeg_fdct_kernel(const EncTables* __restrict__ tables, const uint8_t* __restrict__ rgb,
                                                            int16_t* __restrict__ coef) {
    __shared__ EncCodes T;
    __shared__ int32_t tile[kFdctBlocks][8][kTileStride];
    me_scan::stage_to_lds<kThreads>(T, &tables->c);
    const int local = (int)threadIdx.x >> 3, lane = (int)threadIdx.x & 7;
    const int64_t at = (int64_t)blockIdx.x * kFdctBlocks + local;
    const bool live = at < T.d.total_blocks;
    if (live) fdct_row_lane(T.d, rgb, (int32_t)at, lane, tile[local][lane]);
    __syncthreads();
    if (live) fdct_col_lane(T, (int32_t)at, lane, &tile[local][0][0], kTileStride, coef);
}

// the wave's block, its lane's coefficient and the mask of the non-zero ones; every lane of a wave takes the same branch
__device__ __forceinline__ LaneCode wave_lane_code(const EncCodes& T, const int16_t* coef, int32_t i, int k) {
    const int32_t v = coef[(int64_t)i * 64 + k];
    const uint64_t nz = __ballot(v != 0);
    return lane_code(T, coef, i, k, v, nz);
}

__global__ __launch_bounds__(kThreads) void jpeg_bits_kernel(const EncTables* __restrict__ tables, const int16_t* __restrict__ coef,
                                                            uint32_t* __restrict__ nbits) {
    __shared__ EncCodes T;
    me_scan::stage_to_lds<kThreads>(T, &tables->c);
    const int k = (int)threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaveBlocks + ((int)threadIdx.x >> 6);
    if (i >= T.d.total_blocks) return;  // a whole wave
    const int32_t sum = me_scan::wave_sum(wave_lane_code(T, coef, (int32_t)i, k).len);
    if (k == 0) nbits[i] = (uint32_t)sum;
}

__global__ __launch_bounds__(kThreads) void jpeg_pack_kernel(const EncTables* __restrict__ tables, const int16_t* __restrict__ coef,
                                                            const uint64_t* __restrict__ before, const uint64_t* __restrict__ carry,
                                                            uint32_t* words) {
    __shared__ EncCodes T;
    me_scan::stage_to_lds<kThreads>(T, &tables->c);
    const int k = (int)threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaveBlocks + ((int)threadIdx.x >> 6);
    if (i >= T.d.total_blocks) return;  // a whole wave
    const LaneCode c = wave_lane_code(T, coef, (int32_t)i, k);
    const int32_t incl = me_scan::wave_scan(c.len);  // at most 64 * 59 bits
    const uint64_t at = before[i] + carry[i / kThreads] + (uint64_t)(incl - c.len);
    put_bits(words, at, c.bits, c.len);
    if (i == T.d.total_blocks - 1 && k == 63) {  // the scan's last bit is behind this lane's: ones up to the byte
        const uint64_t end = at + (uint64_t)c.len;
        const int pad = (int)((8 - (end & 7)) & 7);
        put_bits(words, end, (1ull << pad) - 1ull, pad);
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_stuff_count_kernel(const uint32_t* __restrict__ words, int64_t nchunks,
                                                                   uint32_t* __restrict__ counts) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x;
    if (c < nchunks) counts[c] = count_ff(words, c);
}

__global__ __launch_bounds__(kThreads) void jpeg_stuff_kernel(const EncTables* __restrict__ tables, const uint32_t* __restrict__ words,
                                                             int64_t nbytes, int64_t nchunks, const uint64_t* __restrict__ before,
                                                             const uint64_t* __restrict__ carry, uint8_t* __restrict__ file) {
    const int32_t header_len = tables->c.d.header_len;
    if (blockIdx.x == 0)
        for (int k = (int)threadIdx.x; k < header_len; k += kThreads) file[k] = tables->header[k];
    const int64_t c = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x;
    if (c >= nchunks) return;
    stuff_chunk(words, nbytes, c, before[c] + carry[c / kThreads], file + header_len);
    if (c == nchunks - 1) {
        uint8_t* end = file + header_len + nbytes + (int64_t)carry[(nchunks + kThreads - 1) / kThreads];
        end[0] = 0xff, end[1] = 0xd9;
    }
}

// test surface (me_op_exclusive_scan_u32, form 1): the two-level scan's arrays put together as the kernels above read them
__global__ __launch_bounds__(kThreads) void scan_combine_kernel(const uint64_t* __restrict__ before, const uint64_t* __restrict__ carry,
                                                               int64_t n, uint64_t base, uint64_t* __restrict__ offsets) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x;
    if (i < n) offsets[i] = before[i] + carry[i / kThreads] + base;
    if (i == n - 1) offsets[n] = carry[(n + kThreads - 1) / kThreads] + base;
}

}  // namespace

namespace me {

void jpeg_encode_scan_offsets(me_ctx* ctx, const uint32_t* counts, int64_t n, uint64_t base, uint64_t* offsets) {
    const int64_t groups = (int64_t)cdiv(n, kThreads);
    uint64_t* before = (uint64_t*)site_buf(ctx, "op.scan.before", (size_t)n * sizeof(uint64_t));
    uint64_t* agg = (uint64_t*)site_buf(ctx, "op.scan.agg", (size_t)groups * sizeof(uint64_t));
    uint64_t* carry = (uint64_t*)site_buf(ctx, "op.scan.carry", (size_t)(groups + 1) * sizeof(uint64_t));
    me_scan::launch_two_level<kThreads>(counts, n, before, agg, carry, ctx->stream);
    hipLaunchKernelGGL(scan_combine_kernel, dim3((unsigned)groups), dim3(kThreads), 0, ctx->stream, (const uint64_t*)before,
                       (const uint64_t*)carry, n, base, offsets);
    ME_HIP(hipGetLastError());
}

void check_jpeg_encode_args(const char* who, int32_t w, int32_t h, int32_t quality, int32_t subsampling) {
    ME_CHECK(quality >= 1 && quality <= 100, ME_ERR_BAD_ARG, "%s: quality %d outside 1..100", who, quality);
    ME_CHECK(subsampling >= 0 && subsampling <= 2, ME_ERR_BAD_ARG, "%s: subsampling %d (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)", who,
             subsampling);
    constexpr int32_t limit = ME_RESIZE_MAX_DIM < kMaxDim ? ME_RESIZE_MAX_DIM : kMaxDim;
    ME_CHECK(w > 0 && h > 0, ME_ERR_BAD_SHAPE, "%s: %dx%d", who, w, h);
    ME_CHECK(w <= limit && h <= limit, ME_ERR_BAD_SHAPE, "%s: %dx%d: a side exceeds %d", who, w, h, limit);
}

// rgb [h,w,3], host or device -> the file in the context's scratch; synchronises twice (the scan's bits and the file's size
// come back to the host).  Arguments are checked by the caller.
DeviceFile jpeg_encode_device(me_ctx* ctx, const uint8_t* rgb_any, int32_t w, int32_t h, int32_t quality, int32_t subsampling) {
    hipStream_t s = ctx->stream;
    // the output back end may run on its own stream (me_ctx_set_output_overlap): its scratch is its own
    const std::string tag = (ctx->out_stream && s == ctx->out_stream) ? "out.jpegenc." : "jpegenc.";
    JpegEncodeReport& rep = ctx->jpeg_encode_report;
    rep = JpegEncodeReport();
    ctx->jpeg_encode_reported = false;

    std::vector<EncTables> tables(1);
    build_tables(w, h, quality, subsampling, tables[0]);
    const int64_t nblocks = tables[0].c.d.total_blocks;
    const int32_t header_len = tables[0].c.d.header_len;
    const int64_t block_groups = (int64_t)cdiv(nblocks, kThreads);

    EncTables* dtab = (EncTables*)site_buf(ctx, tag + "tables", sizeof(EncTables));
    int16_t* coef = (int16_t*)site_buf(ctx, tag + "coef", (size_t)nblocks * 64 * sizeof(int16_t));
    uint32_t* nbits = (uint32_t*)site_buf(ctx, tag + "nbits", (size_t)nblocks * sizeof(uint32_t));
    uint64_t* before = (uint64_t*)site_buf(ctx, tag + "before", (size_t)nblocks * sizeof(uint64_t));
    uint64_t* agg = (uint64_t*)site_buf(ctx, tag + "agg", (size_t)block_groups * sizeof(uint64_t));
    uint64_t* carry = (uint64_t*)site_buf(ctx, tag + "carry", (size_t)(block_groups + 1) * sizeof(uint64_t));

    ctx->jpeg_encode_marks.record(0, s);
    const uint8_t* rgb = (const uint8_t*)to_device(ctx, rgb_any, (size_t)w * h * 3, tag + "rgb");
    ME_HIP(hipMemcpyAsync(dtab, tables.data(), sizeof(EncTables), hipMemcpyHostToDevice, s));
    ctx->jpeg_encode_marks.record(1, s);
    const int64_t fdct_groups = (int64_t)cdiv(nblocks, kFdctBlocks), wave_groups = (int64_t)cdiv(nblocks, kWaveBlocks);
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)fdct_groups), dim3(kThreads), 0, s, (const EncTables*)dtab, rgb, coef);
    ME_HIP(hipGetLastError());
    ctx->jpeg_encode_marks.record(2, s);
    hipLaunchKernelGGL(jpeg_bits_kernel, dim3((unsigned)wave_groups), dim3(kThreads), 0, s, (const EncTables*)dtab,
                       (const int16_t*)coef, nbits);
    ME_HIP(hipGetLastError());
    me_scan::launch_two_level<kThreads>(nbits, nblocks, before, agg, carry, s);
    ctx->jpeg_encode_marks.record(3, s);
    uint64_t total_bits = 0;
    ME_HIP(hipMemcpyAsync(&total_bits, carry + block_groups, sizeof(total_bits), hipMemcpyDeviceToHost, s));
    ME_HIP(hipStreamSynchronize(s));
    // a block is at least its DC code and an EOB, at most 64 lanes of kMaxLaneBits
    ME_CHECK(total_bits >= (uint64_t)nblocks * 4 && total_bits <= (uint64_t)nblocks * 64 * kMaxLaneBits, ME_ERR_HIP,
             "jpeg encoder: %llu bits counted for %lld blocks", (unsigned long long)total_bits, (long long)nblocks);

    // the packed stream, sized from the counted bits and zero-filled to whole lanes of the stuffing kernels; the file is
    // sized for the worst case of the stuffing: every byte an FF, twice the stream
    const int64_t nbytes = (int64_t)((total_bits + 7) / 8), nchunks = (nbytes + kStuffBytes - 1) / kStuffBytes;
    const int64_t chunk_groups = (int64_t)cdiv(nchunks, kThreads);
    const size_t capacity = (size_t)header_len + 2 * (size_t)nbytes + 2;
    uint32_t* words = (uint32_t*)site_buf(ctx, tag + "words", (size_t)nchunks * kStuffBytes);
    uint32_t* ff = (uint32_t*)site_buf(ctx, tag + "ff", (size_t)nchunks * sizeof(uint32_t));
    uint64_t* ff_before = (uint64_t*)site_buf(ctx, tag + "ff.before", (size_t)nchunks * sizeof(uint64_t));
    uint64_t* ff_agg = (uint64_t*)site_buf(ctx, tag + "ff.agg", (size_t)chunk_groups * sizeof(uint64_t));
    uint64_t* ff_carry = (uint64_t*)site_buf(ctx, tag + "ff.carry", (size_t)(chunk_groups + 1) * sizeof(uint64_t));
    uint8_t* file = (uint8_t*)site_buf(ctx, tag + "file", capacity);
    ME_HIP(hipMemsetAsync(words, 0, (size_t)nchunks * kStuffBytes, s));
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)wave_groups), dim3(kThreads), 0, s, (const EncTables*)dtab,
                       (const int16_t*)coef, (const uint64_t*)before, (const uint64_t*)carry, words);
    ME_HIP(hipGetLastError());
    ctx->jpeg_encode_marks.record(4, s);
    hipLaunchKernelGGL(jpeg_stuff_count_kernel, dim3((unsigned)chunk_groups), dim3(kThreads), 0, s, (const uint32_t*)words, nchunks, ff);
    ME_HIP(hipGetLastError());
    me_scan::launch_two_level<kThreads>(ff, nchunks, ff_before, ff_agg, ff_carry, s);
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)chunk_groups), dim3(kThreads), 0, s, (const EncTables*)dtab,
                       (const uint32_t*)words, nbytes, nchunks, (const uint64_t*)ff_before, (const uint64_t*)ff_carry, file);
    ME_HIP(hipGetLastError());
    ctx->jpeg_encode_marks.record(5, s);
    uint64_t stuffed = 0;
    ME_HIP(hipMemcpyAsync(&stuffed, ff_carry + chunk_groups, sizeof(stuffed), hipMemcpyDeviceToHost, s));
    ME_HIP(hipStreamSynchronize(s));
    ME_CHECK(stuffed <= (uint64_t)nbytes, ME_ERR_HIP, "jpeg encoder: %llu stuffed bytes in a stream of %lld", (unsigned long long)stuffed,
             (long long)nbytes);

    DeviceFile f;
    f.dev = file, f.bytes = (int64_t)header_len + nbytes + (int64_t)stuffed + 2;
    rep.blocks = nblocks, rep.scan_bits = (int64_t)total_bits, rep.stuffed = (int64_t)stuffed, rep.file_bytes = f.bytes;
    rep.fdct_groups = fdct_groups, rep.wave_groups = wave_groups, rep.block_scan_groups = block_groups;
    rep.stuff_groups = chunk_groups, rep.capacity = (int64_t)capacity;
    rep.downloaded = false;
    ctx->jpeg_encode_reported = true;
    return f;
}

void free_jpeg_encode_scratch(me_ctx* ctx) { ctx->jpeg_encode_marks.destroy(); }

}  // namespace me

extern "C" int32_t me_last_jpeg_encode(me_ctx* ctx, int64_t report[10], double ms[6]) {
    ME_API_BEGIN(ctx)
    ME_CHECK(report && ms, ME_ERR_BAD_ARG, "me_last_jpeg_encode: null pointer");
    ME_CHECK(ctx->jpeg_encode_reported, ME_ERR_NOT_READY, "me_last_jpeg_encode: no JPEG encode has completed on this context");
    const JpegEncodeReport& r = ctx->jpeg_encode_report;
    report[0] = r.blocks, report[1] = r.scan_bits, report[2] = r.stuffed, report[3] = r.file_bytes, report[4] = r.fdct_groups;
    report[5] = r.wave_groups, report[6] = r.block_scan_groups, report[7] = r.stuff_groups, report[8] = r.stuff_groups;
    report[9] = r.capacity;
    for (int i = 0; i < 6; ++i) ms[i] = i < 5 || r.downloaded ? ctx->jpeg_encode_marks.ms(i, i + 1) : 0.0;
    ME_API_END(ctx)
}

extern "C" int32_t me_op_jpeg_encode_host(const uint8_t* rgb, int32_t w, int32_t h, int32_t quality, int32_t subsampling,
                                          uint8_t* jpg, int64_t capacity, int64_t* nbytes) {
    if (!rgb || !nbytes || (!jpg && capacity > 0)) return -1;
    try {
        if (w <= 0 || h <= 0) return -2;
        matrix_eyes::RgbImage img((uint32_t)w, (uint32_t)h);
        std::memcpy(img.data.data(), rgb, img.data.size());
        const std::vector<uint8_t> file = matrix_eyes::encode_jpeg(img, quality, subsampling);
        *nbytes = (int64_t)file.size();
        if ((int64_t)file.size() > capacity) return -3;
        std::memcpy(jpg, file.data(), file.size());
    } catch (const std::exception&) {
        return -2;
    }
    return 0;
}
