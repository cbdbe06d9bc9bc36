// The clamp, raster and file entries of the output back end (include/matrix_eyes_hip.h): the stereogram and the colour map of
// output.rs:123-193 as pictures, and RgbImage::save (:138, :192) of either, or of a caller's picture, to a PNG or JPEG file
// encoded on the device.  Host code only: the kernels are those of output.hip, resample.hip, png_encode.hip and
// jpeg_encode.hip, and every chain of them is spelled out once here.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <sys/random.h>

#include "chacha.h"
#include "model.h"

using namespace me;

namespace {

// The noise of a stereogram: a caller's [out_h][out_w][3] picture (host or device), or the 32-byte key (host memory) of the
// keyed entries, from which the fill kernel makes that picture in the context's scratch
struct NoiseSource {
    const uint8_t* noise = nullptr;
    const uint8_t* key = nullptr;
    explicit operator bool() const { return noise || key; }
};
NoiseSource from_buffer(const uint8_t* noise) { return NoiseSource{noise, nullptr}; }
NoiseSource from_key(const uint8_t* key) { return NoiseSource{nullptr, key}; }

// output.rs:141-190 into dst_dev [out_h][out_w][3]; range_dev: the depth's range in device memory, in place of the two numbers
void render_stereogram(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth, float max_depth,
                       const float* range_dev, int32_t out_w, int32_t out_h, float amplitude, NoiseSource src,
                       uint8_t* dst_dev) {
    const float* d = (const float*)to_device(ctx, depth, (size_t)rows * cols * 4, "out.depth");
    if (src.key)
        return stereogram_keyed_launch(ctx, d, rows, cols, min_depth, max_depth, range_dev, out_w, out_h, amplitude, src.key, dst_dev);
    const uint8_t* nz = (const uint8_t*)to_device(ctx, src.noise, (size_t)out_w * out_h * 3, "out.noise");
    stereogram_launch(d, rows, cols, min_depth, max_depth, range_dev, out_w, out_h, amplitude, nz, dst_dev, ctx->stream);
}

// output.rs:124-131 the colour map in data order (RgbImage::new(data_width, data_height)), :133-137 the resize into
// dst_dev [out_h][out_w][3]
void render_depth_map(me_ctx* ctx, const char* who, const float* depth, int32_t data_width, int32_t data_height, float min_depth,
                      float max_depth, const float* minmax_dev, int32_t out_w, int32_t out_h, uint8_t* dst_dev) {
    const int64_t count = (int64_t)data_width * data_height;
    const float* d = (const float*)to_device(ctx, depth, (size_t)count * 4, "out.depth");
    uint8_t* mapped = (uint8_t*)site_buf(ctx, "out.rgb.native", (size_t)count * 3);
    depthmap_rgb_launch(d, count, min_depth, max_depth, minmax_dev, mapped, ctx->stream);
    ME_CHECK(dst_dev != mapped, ME_ERR_BAD_ARG, "%s: rgb is the context's own scratch", who);
    resize_lanczos3_rgb8(ctx, mapped, data_width, data_height, dst_dev, out_w, out_h);
}

// the file to the host in one copy, then to `path`; after_copy is recorded behind the copy
void write_device_file(me_ctx* ctx, const DeviceFile& f, const char* path, hipEvent_t after_copy = nullptr) {
    std::vector<uint8_t> host((size_t)f.bytes);
    ME_HIP(hipMemcpyAsync(host.data(), f.dev, host.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (after_copy) ME_HIP(hipEventRecord(after_copy, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    FILE* fp = fopen(path, "wb");
    ME_CHECK(fp, ME_ERR_IO, "cannot create %s: %s", path, strerror(errno));
    const bool ok = fwrite(host.data(), 1, host.size(), fp) == host.size();
    const int werr = errno;
    const int r = fclose(fp);
    ME_CHECK(ok, ME_ERR_IO, "write failed: %s: %s", path, strerror(werr));
    ME_CHECK(r == 0, ME_ERR_IO, "close failed: %s: %s", path, strerror(errno));
}

// the JPEG file of a picture to `path`: the download is the encode's sixth leg (me_last_jpeg_encode)
void write_jpeg(me_ctx* ctx, const uint8_t* rgb_any, int32_t w, int32_t h, int32_t quality, int32_t subsampling, const char* path) {
    const DeviceFile f = jpeg_encode_device(ctx, rgb_any, w, h, quality, subsampling);
    ctx->jpeg_encode_report.downloaded = true;
    write_device_file(ctx, f, path, ctx->jpeg_encode_marks.at(6));
}

void stereogram_impl(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth, float max_depth,
                     const float* range_dev, int32_t out_w, int32_t out_h, float amplitude, NoiseSource noise,
                     uint8_t* out) {
    ME_CHECK(depth && noise && out, ME_ERR_BAD_ARG, "me_stereogram: null pointer");
    ME_CHECK(rows > 0 && cols > 0 && out_w > 0 && out_h > 0, ME_ERR_BAD_SHAPE,
             "me_stereogram: %dx%d -> %dx%d", rows, cols, out_w, out_h);
    OutBuf o = out_buf(ctx, out, (size_t)out_w * out_h * 3, "out.stereo");
    render_stereogram(ctx, depth, rows, cols, min_depth, max_depth, range_dev, out_w, out_h, amplitude, noise, (uint8_t*)o.dev);
    finish(ctx, o);
}

// output.rs:141-193 whole, to a ".png" (who: the entry's name)
void output_stereogram_png_impl(me_ctx* ctx, const char* who, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                float max_depth, int32_t out_w, int32_t out_h, float amplitude, NoiseSource noise,
                                const char* destination_path) {
    ME_CHECK(depth && noise && destination_path, ME_ERR_BAD_ARG, "%s: null pointer", who);
    ME_CHECK(rows > 0 && cols > 0, ME_ERR_BAD_SHAPE, "%s: %dx%d -> %dx%d", who, rows, cols, out_w, out_h);
    check_png_shape(who, out_w, out_h);
    uint8_t* rgb = (uint8_t*)site_buf(ctx, "out.stereo", (size_t)out_w * out_h * 3);
    render_stereogram(ctx, depth, rows, cols, min_depth, max_depth, nullptr, out_w, out_h, amplitude, noise, rgb);
    write_device_file(ctx, png_encode_device(ctx, rgb, out_w, out_h), destination_path);
}

// ... and to a ".jpg"
void output_stereogram_jpeg_impl(me_ctx* ctx, const char* who, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                 float max_depth, int32_t out_w, int32_t out_h, float amplitude, NoiseSource noise,
                                 int32_t quality, int32_t subsampling, const char* destination_path) {
    ME_CHECK(depth && noise && destination_path, ME_ERR_BAD_ARG, "%s: null pointer", who);
    ME_CHECK(rows > 0 && cols > 0, ME_ERR_BAD_SHAPE, "%s: %dx%d -> %dx%d", who, rows, cols, out_w, out_h);
    check_jpeg_encode_args(who, out_w, out_h, quality, subsampling);
    uint8_t* rgb = (uint8_t*)site_buf(ctx, "out.stereo", (size_t)out_w * out_h * 3);
    render_stereogram(ctx, depth, rows, cols, min_depth, max_depth, nullptr, out_w, out_h, amplitude, noise, rgb);
    write_jpeg(ctx, rgb, out_w, out_h, quality, subsampling, destination_path);
}

void depthmap_rgb_impl(me_ctx* ctx, const float* depth, int64_t count, float min_depth, float max_depth,
                       const float* range_dev, uint8_t* rgb) {
    ME_CHECK(depth && rgb && count > 0, ME_ERR_BAD_ARG, "me_depthmap_rgb: bad argument");
    const float* d = (const float*)to_device(ctx, depth, (size_t)count * 4, "out.depth");
    OutBuf o = out_buf(ctx, rgb, (size_t)count * 3, "out.rgb");
    depthmap_rgb_launch(d, count, min_depth, max_depth, range_dev, (uint8_t*)o.dev, ctx->stream);
    finish(ctx, o);
}

}  // namespace

extern "C" {

// ---- the clamp every output starts from (output.rs:51-62) ----------------------------------------------------------
int32_t me_depth_clamp_minmax(me_ctx* ctx, float* depth, int64_t count, float* min_out,
                              float* max_out) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && count > 0, ME_ERR_BAD_ARG, "me_depth_clamp_minmax: bad argument");
    const bool dev = is_device_ptr(depth);
    float* d = dev ? depth : (float*)site_buf(ctx, "out.depth", (size_t)count * 4);
    if (!dev) ME_HIP(hipMemcpyAsync(d, depth, (size_t)count * 4, hipMemcpyHostToDevice, ctx->stream));
    float* mm = (float*)site_buf(ctx, "out.minmax", 8);
    depth_clamp_minmax_launch(d, count, mm, ctx->stream);
    float host[2];
    ME_HIP(hipMemcpyAsync(host, mm, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!dev) ME_HIP(hipMemcpyAsync(depth, d, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    if (min_out) *min_out = host[0];
    if (max_out) *max_out = host[1];
    ME_API_END(ctx)
}

int32_t me_depth_clamp_minmax_async(me_ctx* ctx, float* depth, int64_t count, float* minmax_dev) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && minmax_dev && count > 0, ME_ERR_BAD_ARG, "me_depth_clamp_minmax_async: bad argument");
    ME_CHECK(is_device_ptr(depth) && is_device_ptr(minmax_dev), ME_ERR_BAD_ARG,
             "me_depth_clamp_minmax_async: depth and minmax_dev must be device memory");
    depth_clamp_minmax_launch(depth, count, minmax_dev, ctx->stream);
    ME_API_END(ctx)
}

int32_t me_stereogram(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                      float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                      const uint8_t* noise, uint8_t* out) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    stereogram_impl(ctx, depth, rows, cols, min_depth, max_depth, nullptr, out_w, out_h, amplitude, from_buffer(noise), out);
    ME_API_END(ctx)
}

int32_t me_stereogram_dev_range(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols,
                                const float* minmax_dev, int32_t out_w, int32_t out_h, float amplitude,
                                const uint8_t* noise, uint8_t* out) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(minmax_dev && is_device_ptr(minmax_dev), ME_ERR_BAD_ARG, "me_stereogram_dev_range: minmax_dev");
    stereogram_impl(ctx, depth, rows, cols, 0.f, 0.f, minmax_dev, out_w, out_h, amplitude, from_buffer(noise), out);
    ME_API_END(ctx)
}

// ---- the keyed noise (chacha.h, stereogram_noise.hip) --------------------------------------------------------------
int32_t me_noise_key_from_seed(uint64_t seed, uint8_t key[32]) {
    if (!key) {
        create_error() = "me_noise_key_from_seed: null pointer";
        return ME_ERR_BAD_ARG;
    }
    me_chacha::key_from_seed(seed, key);
    return ME_OK;
}

int32_t me_noise_key_from_os(uint8_t key[32]) {
    if (!key) {
        create_error() = "me_noise_key_from_os: null pointer";
        return ME_ERR_BAD_ARG;
    }
    for (size_t have = 0; have < 32;) {
        const ssize_t n = getrandom(key + have, 32 - have, 0);
        if (n < 0 && errno == EINTR) continue;
        if (n <= 0) {
            create_error() = std::string("me_noise_key_from_os: getrandom: ") + strerror(errno);
            return ME_ERR_IO;
        }
        have += (size_t)n;
    }
    return ME_OK;
}

int32_t me_stereogram_noise_host(const uint8_t key[32], int32_t out_w, int32_t out_h, uint8_t* out) {
    if (!key || !out) {
        create_error() = "me_stereogram_noise_host: null pointer";
        return ME_ERR_BAD_ARG;
    }
    if (out_w <= 0 || out_h <= 0) {
        create_error() = "me_stereogram_noise_host: " + std::to_string(out_w) + "x" + std::to_string(out_h);
        return ME_ERR_BAD_SHAPE;
    }
    me_chacha::noise_fill_host(key, out_w, out_h, out);
    return ME_OK;
}

int32_t me_op_legacy_noise_host(uint32_t seed, int64_t nbytes, uint8_t* out) {
    if (!out || nbytes < 0) {
        create_error() = "me_op_legacy_noise_host: bad argument";
        return ME_ERR_BAD_ARG;
    }
    // host/matrix_eyes.cpp DepthMap::output_stereogram, its loop as written there
    std::mt19937 rng(seed);
    const size_t n = (size_t)nbytes;
    for (size_t i = 0; i < n; i += 4) {
        const uint32_t v = rng();
        for (size_t k = 0; k < 4 && i + k < n; ++k) out[i + k] = (uint8_t)(v >> (8 * k));
    }
    return ME_OK;
}

int32_t me_stereogram_noise(me_ctx* ctx, const uint8_t key[32], int32_t out_w, int32_t out_h, uint8_t* out) {
    ME_API_BEGIN(ctx)
    ME_CHECK(key && out, ME_ERR_BAD_ARG, "me_stereogram_noise: null pointer");
    ME_CHECK(out_w > 0 && out_h > 0, ME_ERR_BAD_SHAPE, "me_stereogram_noise: %dx%d", out_w, out_h);
    ME_CHECK(out_w <= 16384, ME_ERR_BAD_SHAPE, "me_stereogram_noise: width %d > 16384", out_w);
    OutBuf o = out_buf(ctx, out, (size_t)out_w * out_h * 3, "out.noise");
    stereogram_noise_fill_launch(ctx, key, out_w, out_h, (uint8_t*)o.dev, 1);
    finish(ctx, o);
    ME_API_END(ctx)
}

int32_t me_stereogram_keyed(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth, float max_depth,
                            int32_t out_w, int32_t out_h, float amplitude, const uint8_t key[32], uint8_t* out) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    stereogram_impl(ctx, depth, rows, cols, min_depth, max_depth, nullptr, out_w, out_h, amplitude, from_key(key), out);
    ME_API_END(ctx)
}

int32_t me_stereogram_keyed_dev_range(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, const float* minmax_dev,
                                      int32_t out_w, int32_t out_h, float amplitude, const uint8_t key[32], uint8_t* out) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(minmax_dev && is_device_ptr(minmax_dev), ME_ERR_BAD_ARG, "me_stereogram_keyed_dev_range: minmax_dev");
    stereogram_impl(ctx, depth, rows, cols, 0.f, 0.f, minmax_dev, out_w, out_h, amplitude, from_key(key), out);
    ME_API_END(ctx)
}

int32_t me_last_stereogram_noise(me_ctx* ctx, int64_t report[2], double* kernel_ms) {
    ME_API_BEGIN(ctx)
    ME_CHECK(report && kernel_ms, ME_ERR_BAD_ARG, "me_last_stereogram_noise: null pointer");
    ME_CHECK(ctx->stereo_noise_path != 0, ME_ERR_NOT_READY, "me_last_stereogram_noise: no keyed noise has been made on this context");
    ME_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->out_stream) ME_HIP(hipStreamSynchronize(ctx->out_stream));
    report[0] = ctx->stereo_noise_path, report[1] = ctx->stereo_noise_words;
    *kernel_ms = ctx->stereo_noise_marks.ms(0, 1);
    ME_API_END(ctx)
}

int32_t me_depthmap_rgb(me_ctx* ctx, const float* depth, int64_t count, float min_depth,
                        float max_depth, uint8_t* rgb) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    depthmap_rgb_impl(ctx, depth, count, min_depth, max_depth, nullptr, rgb);
    ME_API_END(ctx)
}

int32_t me_depthmap_rgb_dev_range(me_ctx* ctx, const float* depth, int64_t count, const float* minmax_dev,
                                  uint8_t* rgb) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(minmax_dev && is_device_ptr(minmax_dev), ME_ERR_BAD_ARG, "me_depthmap_rgb_dev_range: minmax_dev");
    depthmap_rgb_impl(ctx, depth, count, 0.f, 0.f, minmax_dev, rgb);
    ME_API_END(ctx)
}

int32_t me_depthmap_rgb_resized(me_ctx* ctx, const float* depth, int32_t data_width, int32_t data_height,
                                float min_depth, float max_depth, const float* minmax_dev, int32_t out_w,
                                int32_t out_h, uint8_t* rgb) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && rgb, ME_ERR_BAD_ARG, "me_depthmap_rgb_resized: null pointer");
    ME_CHECK(!minmax_dev || is_device_ptr(minmax_dev), ME_ERR_BAD_ARG, "me_depthmap_rgb_resized: minmax_dev");
    check_resize_shape("me_depthmap_rgb_resized", data_width, data_height, out_w, out_h);
    OutBuf o = out_buf(ctx, rgb, (size_t)out_w * out_h * 3, "out.rgb");
    render_depth_map(ctx, "me_depthmap_rgb_resized", depth, data_width, data_height, min_depth, max_depth, minmax_dev, out_w, out_h,
                     (uint8_t*)o.dev);
    finish(ctx, o);
    ME_API_END(ctx)
}

// ---- PNG files (png_encode.hip) ------------------------------------------------------------------------------------
int32_t me_png_encode_rgb8(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, const uint8_t** png_dev, int64_t* nbytes) {
    ME_API_BEGIN(ctx)
    ME_CHECK(rgb && png_dev && nbytes, ME_ERR_BAD_ARG, "me_png_encode_rgb8: null pointer");
    check_png_shape("me_png_encode_rgb8", w, h);
    OutputScope out_scope(ctx, is_device_ptr(rgb) ? rgb : nullptr);
    const uint8_t* d = (const uint8_t*)to_device(ctx, rgb, (size_t)w * h * 3, "png.rgb");
    const DeviceFile f = png_encode_device(ctx, d, w, h);
    *png_dev = f.dev, *nbytes = f.bytes;
    ME_API_END(ctx)
}

int32_t me_output_png(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, const char* destination_path) {
    ME_API_BEGIN(ctx)
    ME_CHECK(rgb && destination_path, ME_ERR_BAD_ARG, "me_output_png: null pointer");
    check_png_shape("me_output_png", w, h);
    OutputScope out_scope(ctx, is_device_ptr(rgb) ? rgb : nullptr);
    const uint8_t* d = (const uint8_t*)to_device(ctx, rgb, (size_t)w * h * 3, "png.rgb");
    write_device_file(ctx, png_encode_device(ctx, d, w, h), destination_path);
    ME_API_END(ctx)
}

int32_t me_output_depth_map_png(me_ctx* ctx, const float* depth, int32_t data_width, int32_t data_height,
                                float min_depth, float max_depth, const float* minmax_dev, int32_t out_w,
                                int32_t out_h, const char* destination_path) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && destination_path, ME_ERR_BAD_ARG, "me_output_depth_map_png: null pointer");
    ME_CHECK(!minmax_dev || is_device_ptr(minmax_dev), ME_ERR_BAD_ARG, "me_output_depth_map_png: minmax_dev");
    check_png_shape("me_output_depth_map_png", data_width, data_height);
    check_png_shape("me_output_depth_map_png", out_w, out_h);
    uint8_t* rgb = (uint8_t*)site_buf(ctx, "out.rgb", (size_t)out_w * out_h * 3);
    render_depth_map(ctx, "me_output_depth_map_png", depth, data_width, data_height, min_depth, max_depth, minmax_dev, out_w, out_h, rgb);
    write_device_file(ctx, png_encode_device(ctx, rgb, out_w, out_h), destination_path);
    ME_API_END(ctx)
}

int32_t me_output_stereogram_png(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                 float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                 const uint8_t* noise, const char* destination_path) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    output_stereogram_png_impl(ctx, "me_output_stereogram_png", depth, rows, cols, min_depth, max_depth, out_w, out_h, amplitude,
                               from_buffer(noise), destination_path);
    ME_API_END(ctx)
}

int32_t me_output_stereogram_png_keyed(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                       float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                       const uint8_t key[32], const char* destination_path) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    output_stereogram_png_impl(ctx, "me_output_stereogram_png_keyed", depth, rows, cols, min_depth, max_depth, out_w, out_h,
                               amplitude, from_key(key), destination_path);
    ME_API_END(ctx)
}

// ---- JPEG files (jpeg_encode.hip) ----------------------------------------------------------------------------------
int32_t me_jpeg_encode_rgb8(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, int32_t quality, int32_t subsampling,
                            const uint8_t** jpg_dev, int64_t* nbytes) {
    ME_API_BEGIN(ctx)
    ME_CHECK(rgb && jpg_dev && nbytes, ME_ERR_BAD_ARG, "me_jpeg_encode_rgb8: null pointer");
    check_jpeg_encode_args("me_jpeg_encode_rgb8", w, h, quality, subsampling);
    OutputScope out_scope(ctx, is_device_ptr(rgb) ? rgb : nullptr);
    const DeviceFile f = jpeg_encode_device(ctx, rgb, w, h, quality, subsampling);
    *jpg_dev = f.dev, *nbytes = f.bytes;
    ME_API_END(ctx)
}

int32_t me_output_jpeg(me_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, int32_t quality, int32_t subsampling,
                       const char* destination_path) {
    ME_API_BEGIN(ctx)
    ME_CHECK(rgb && destination_path, ME_ERR_BAD_ARG, "me_output_jpeg: null pointer");
    check_jpeg_encode_args("me_output_jpeg", w, h, quality, subsampling);
    OutputScope out_scope(ctx, is_device_ptr(rgb) ? rgb : nullptr);
    write_jpeg(ctx, rgb, w, h, quality, subsampling, destination_path);
    ME_API_END(ctx)
}

int32_t me_output_depth_map_jpeg(me_ctx* ctx, const float* depth, int32_t data_width, int32_t data_height,
                                 float min_depth, float max_depth, const float* minmax_dev, int32_t out_w,
                                 int32_t out_h, int32_t quality, int32_t subsampling, const char* destination_path) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && destination_path, ME_ERR_BAD_ARG, "me_output_depth_map_jpeg: null pointer");
    ME_CHECK(!minmax_dev || is_device_ptr(minmax_dev), ME_ERR_BAD_ARG, "me_output_depth_map_jpeg: minmax_dev");
    check_jpeg_encode_args("me_output_depth_map_jpeg", data_width, data_height, quality, subsampling);
    check_jpeg_encode_args("me_output_depth_map_jpeg", out_w, out_h, quality, subsampling);
    uint8_t* rgb = (uint8_t*)site_buf(ctx, "out.rgb", (size_t)out_w * out_h * 3);
    render_depth_map(ctx, "me_output_depth_map_jpeg", depth, data_width, data_height, min_depth, max_depth, minmax_dev, out_w, out_h, rgb);
    write_jpeg(ctx, rgb, out_w, out_h, quality, subsampling, destination_path);
    ME_API_END(ctx)
}

int32_t me_output_stereogram_jpeg(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                  float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                  const uint8_t* noise, int32_t quality, int32_t subsampling,
                                  const char* destination_path) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    output_stereogram_jpeg_impl(ctx, "me_output_stereogram_jpeg", depth, rows, cols, min_depth, max_depth, out_w, out_h, amplitude,
                                from_buffer(noise), quality, subsampling, destination_path);
    ME_API_END(ctx)
}

int32_t me_output_stereogram_jpeg_keyed(me_ctx* ctx, const float* depth, int32_t rows, int32_t cols, float min_depth,
                                        float max_depth, int32_t out_w, int32_t out_h, float amplitude,
                                        const uint8_t key[32], int32_t quality, int32_t subsampling,
                                        const char* destination_path) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    output_stereogram_jpeg_impl(ctx, "me_output_stereogram_jpeg_keyed", depth, rows, cols, min_depth, max_depth, out_w, out_h,
                                amplitude, from_key(key), quality, subsampling, destination_path);
    ME_API_END(ctx)
}

}  // extern "C"
