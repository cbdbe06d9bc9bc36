// The photo-input entries (include/matrix_eyes_hip.h, matrix_eyes_hip_ops.h), the counterpart of output_api.hip: a JPEG or
// PNG file in host memory -> its header, its oriented RGB picture, or that picture resized for the model, and the Lanczos3
// resize alone.  Host code only: the kernels are those of jpeg_decode.hip, jpeg_entropy.hip, png_decode.hip and resample.hip.
// What the two formats share is spelled out once, over a codec descriptor; a further format is one more descriptor.
#include <cstring>
#include <exception>
#include <vector>

#include "../../include/matrix_eyes_hip_ops.h"
#include "../host/image_io.hpp"
#include "model.h"

using namespace me;

namespace {

struct PhotoHead {
    int32_t width, height;
    int64_t exif_offset, exif_nbytes;
};

struct Codec {
    const char* tag;       // the file's name in the decoders' messages (the host layer rewrites it into the path)
    const char* word;      // the format in this unit's messages
    const char* resized;   // site buffer of a resized picture bound for a host destination
    PhotoHead (*head)(const std::vector<uint8_t>& file, const char* tag);
    matrix_eyes::RgbImage (*decode_host)(const std::vector<uint8_t>& file, const std::string& path, std::vector<uint8_t>* exif);
    uint8_t* (*decode)(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst_dev, int32_t want_w,
                       int32_t want_h, int32_t* ow, int32_t* oh);
    void (*mark_download)(me_ctx* ctx);   // the mark behind the copy of the picture to the host, the decode's last leg
};

PhotoHead jpeg_head(const std::vector<uint8_t>& file, const char* tag) {
    const matrix_eyes::JpegCoefficients h = matrix_eyes::parse_jpeg_header(file, tag);
    return {h.width, h.height, (int64_t)h.exif_offset, (int64_t)h.exif_nbytes};
}
PhotoHead png_head(const std::vector<uint8_t>& file, const char* tag) {
    const matrix_eyes::PngFrame h = matrix_eyes::parse_png_header(file, tag);
    return {(int32_t)h.width, (int32_t)h.height, (int64_t)h.exif_offset, (int64_t)h.exif_nbytes};
}
void jpeg_mark_download(me_ctx* ctx) {
    ctx->jpeg_marks.record(4, ctx->stream);
    ctx->jpeg_timed_download = true;
}
void png_mark_download(me_ctx* ctx) {
    ctx->png_marks.record(3 * (size_t)ctx->png_timed_bands + 2, ctx->stream);
    ctx->png_timed_download = true;
}

const Codec kJpeg = {"<jpeg>", "JPEG", "jpeg.resized", jpeg_head, matrix_eyes::decode_jpeg, jpeg_decode_rgb8, jpeg_mark_download};
const Codec kPng = {"<png>", "PNG", "png.resized", png_head, matrix_eyes::decode_png, png_decode_rgb8, png_mark_download};

int32_t photo_info(const Codec& c, const char* who, const uint8_t* file, int64_t nbytes, int32_t* width, int32_t* height,
                   int64_t* exif_offset, int64_t* exif_nbytes) {
    if (!file || nbytes < 0 || !width || !height || !exif_offset || !exif_nbytes) {
        create_error() = std::string(who) + ": null pointer";
        return ME_ERR_BAD_ARG;
    }
    try {
        const PhotoHead head = c.head(std::vector<uint8_t>(file, file + nbytes), c.tag);
        *width = head.width, *height = head.height;
        *exif_offset = head.exif_offset, *exif_nbytes = head.exif_nbytes;
    } catch (const std::exception& e) {
        create_error() = e.what();
        return ME_ERR_BAD_ARG;
    }
    return ME_OK;
}

int32_t photo_decode_host(const Codec& c, const uint8_t* file, int64_t nbytes, uint8_t* rgb, int32_t w, int32_t h) {
    if (!file || nbytes < 0 || !rgb) return -1;
    try {
        const matrix_eyes::RgbImage img = c.decode_host(std::vector<uint8_t>(file, file + nbytes), c.tag, nullptr);
        if ((int64_t)img.width != w || (int64_t)img.height != h) return -2;
        std::memcpy(rgb, img.data.data(), img.data.size());
    } catch (const std::exception& e) {
        create_error() = e.what();
        return -3;
    }
    return 0;
}

void check_photo_args(const char* who, const uint8_t* file, int64_t nbytes, int32_t orientation, const void* dst) {
    ME_CHECK(file && dst && nbytes >= 0, ME_ERR_BAD_ARG, "%s: null pointer", who);
    ME_CHECK(orientation >= 1 && orientation <= 8, ME_ERR_BAD_ARG, "%s: orientation %d outside 1..8", who, orientation);
    ME_CHECK(!is_device_ptr(file), ME_ERR_BAD_ARG, "%s: the file's bytes must be in host memory (they are parsed there)", who);
}

int32_t photo_decode(const Codec& c, const char* who, me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation,
                     uint8_t* rgb, int32_t w, int32_t h) {
    ME_API_BEGIN(ctx)
    check_photo_args(who, file, nbytes, orientation, rgb);
    ME_CHECK(w > 0 && h > 0, ME_ERR_BAD_SHAPE, "%s: %dx%d", who, w, h);
    const size_t nout = (size_t)w * h * 3;
    const bool dev = is_device_ptr(rgb);
    int32_t ow = 0, oh = 0;
    uint8_t* d = c.decode(ctx, file, nbytes, orientation, dev ? rgb : nullptr, w, h, &ow, &oh);
    if (!dev) {
        ME_HIP(hipMemcpyAsync(rgb, d, nout, hipMemcpyDeviceToHost, ctx->stream));
        c.mark_download(ctx);
        ME_HIP(hipStreamSynchronize(ctx->stream));
    }
    ME_API_END(ctx)
}

int32_t photo_decode_resized(const Codec& c, const char* who, me_ctx* ctx, const uint8_t* file, int64_t nbytes,
                             int32_t orientation, uint8_t* dst, int32_t nw, int32_t nh) {
    ME_API_BEGIN(ctx)
    check_photo_args(who, file, nbytes, orientation, dst);
    ME_CHECK(nw > 0 && nh > 0 && nw <= ME_RESIZE_MAX_DIM && nh <= ME_RESIZE_MAX_DIM, ME_ERR_BAD_SHAPE, "%s: -> %dx%d", who, nw, nh);
    {
        int32_t fw = 0, fh = 0;  // the file's size before anything is decoded: the resampler's bound
        int64_t eo = 0, en = 0;
        if (photo_info(c, who, file, nbytes, &fw, &fh, &eo, &en) != ME_OK) fail(ME_ERR_BAD_ARG, "%s", create_error().c_str());
        check_resize_shape(who, fw, fh, nw, nh);
    }
    int32_t ow = 0, oh = 0;
    const uint8_t* full = c.decode(ctx, file, nbytes, orientation, nullptr, 0, 0, &ow, &oh);
    OutBuf o = out_buf(ctx, dst, (size_t)nw * nh * 3, c.resized);
    resize_lanczos3_rgb8(ctx, full, ow, oh, (uint8_t*)o.dev, nw, nh);
    finish(ctx, o);
    ME_API_END(ctx)
}

// what both timing reports start with; on return the stream is idle and the marks can be read
void timing_ready(const Codec& c, const char* who, me_ctx* ctx, const double* ms_out, bool timed) {
    ME_CHECK(ms_out, ME_ERR_BAD_ARG, "%s: null pointer", who);
    ME_CHECK(timed, ME_ERR_NOT_READY, "%s: no %s decode has completed on this context", who, c.word);
    ME_HIP(hipStreamSynchronize(ctx->stream));
}

}  // namespace

extern "C" {

int32_t me_resize_lanczos3_rgb8(me_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst, int32_t nw,
                                int32_t nh) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src && dst, ME_ERR_BAD_ARG, "me_resize_lanczos3_rgb8: null pointer");
    check_resize_shape("me_resize_lanczos3_rgb8", w, h, nw, nh);
    const size_t nin = (size_t)w * h * 3, nout = (size_t)nw * nh * 3;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    ME_CHECK(a + nin <= b || b + nout <= a, ME_ERR_BAD_ARG, "me_resize_lanczos3_rgb8: src and dst overlap");
    const uint8_t* s = (const uint8_t*)to_device(ctx, src, nin, "resample.src");
    OutBuf o = out_buf(ctx, dst, nout, "resample.dst");
    resize_lanczos3_rgb8(ctx, s, w, h, (uint8_t*)o.dev, nw, nh);
    finish(ctx, o);
    ME_API_END(ctx)
}

// ---- JPEG (jpeg_decode.hip) and PNG (png_decode.hip) decoding -------------------------------------------------------------
int32_t me_jpeg_info(const uint8_t* file, int64_t nbytes, int32_t* width, int32_t* height, int64_t* exif_offset,
                     int64_t* exif_nbytes) {
    return photo_info(kJpeg, "me_jpeg_info", file, nbytes, width, height, exif_offset, exif_nbytes);
}
int32_t me_png_info(const uint8_t* file, int64_t nbytes, int32_t* width, int32_t* height, int64_t* exif_offset,
                    int64_t* exif_nbytes) {
    return photo_info(kPng, "me_png_info", file, nbytes, width, height, exif_offset, exif_nbytes);
}

int32_t me_op_jpeg_decode_host(const uint8_t* file, int64_t nbytes, uint8_t* rgb, int32_t w, int32_t h) {
    return photo_decode_host(kJpeg, file, nbytes, rgb, w, h);
}
int32_t me_op_png_decode_host(const uint8_t* file, int64_t nbytes, uint8_t* rgb, int32_t w, int32_t h) {
    return photo_decode_host(kPng, file, nbytes, rgb, w, h);
}

int32_t me_jpeg_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* rgb, int32_t w,
                            int32_t h) {
    return photo_decode(kJpeg, "me_jpeg_decode_rgb8", ctx, file, nbytes, orientation, rgb, w, h);
}
int32_t me_png_decode_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* rgb, int32_t w,
                           int32_t h) {
    return photo_decode(kPng, "me_png_decode_rgb8", ctx, file, nbytes, orientation, rgb, w, h);
}

int32_t me_jpeg_decode_resized_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst,
                                    int32_t nw, int32_t nh) {
    return photo_decode_resized(kJpeg, "me_jpeg_decode_resized_rgb8", ctx, file, nbytes, orientation, dst, nw, nh);
}
int32_t me_png_decode_resized_rgb8(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t orientation, uint8_t* dst,
                                   int32_t nw, int32_t nh) {
    return photo_decode_resized(kPng, "me_png_decode_resized_rgb8", ctx, file, nbytes, orientation, dst, nw, nh);
}

// [0] the host's leg (wall clock), then upload, first kernel leg, finish kernel and download between the decode's marks;
// the two decoders place their marks differently (one upload against one per band)
int32_t me_last_jpeg_timing(me_ctx* ctx, double ms_out[5]) {
    ME_API_BEGIN(ctx)
    timing_ready(kJpeg, "me_last_jpeg_timing", ctx, ms_out, ctx->jpeg_timed);
    ms_out[0] = ctx->jpeg_entropy_ms;
    for (int i = 0; i < 4; ++i) ms_out[1 + i] = i < 3 || ctx->jpeg_timed_download ? ctx->jpeg_marks.ms(i, i + 1) : 0.0;
    ME_API_END(ctx)
}
int32_t me_last_png_timing(me_ctx* ctx, double ms_out[5]) {
    ME_API_BEGIN(ctx)
    timing_ready(kPng, "me_last_png_timing", ctx, ms_out, ctx->png_timed);
    ms_out[0] = ctx->png_inflate_ms;
    for (int i = 1; i < 5; ++i) ms_out[i] = 0.0;
    me::LegMarks& m = ctx->png_marks;
    const size_t bands = (size_t)ctx->png_timed_bands;
    for (size_t i = 0; i < bands; ++i) ms_out[1] += m.ms(3 * i, 3 * i + 1), ms_out[2] += m.ms(3 * i + 1, 3 * i + 2);
    ms_out[3] = m.ms(3 * bands, 3 * bands + 1);
    if (ctx->png_timed_download) ms_out[4] = m.ms(3 * bands + 1, 3 * bands + 2);
    ME_API_END(ctx)
}

int32_t me_op_png_unfilter(me_ctx* ctx, const uint8_t* stream, int64_t nbytes, int32_t width, int32_t height, int32_t bit_depth,
                           int32_t colour_type, int32_t interlace, int32_t band_rows, uint8_t* out) {
    ME_API_BEGIN(ctx)
    ME_CHECK(stream && out && nbytes >= 0, ME_ERR_BAD_ARG, "me_op_png_unfilter: null pointer");
    ME_CHECK(width > 0 && height > 0 && (int64_t)width * height <= matrix_eyes::kMaxPixels, ME_ERR_BAD_SHAPE, "me_op_png_unfilter: %dx%d",
             width, height);
    const bool depth_ok = bit_depth == 1 || bit_depth == 2 || bit_depth == 4 || bit_depth == 8 || bit_depth == 16;
    ME_CHECK(depth_ok && me_pngdec::channels_of(colour_type) && !(bit_depth < 8 && colour_type != 0 && colour_type != 3) &&
                 !(bit_depth == 16 && colour_type == 3) && (interlace == 0 || interlace == 1) && band_rows >= 0,
             ME_ERR_BAD_ARG, "me_op_png_unfilter: depth %d, colour type %d, interlace %d, band_rows %d", bit_depth, colour_type, interlace,
             band_rows);
    const me_pngdec::Geom g = me_pngdec::make_geom(width, height, bit_depth, colour_type, interlace);
    ME_CHECK(nbytes == g.total, ME_ERR_BAD_SHAPE, "me_op_png_unfilter: the stream of this picture has %lld bytes, not %lld",
             (long long)g.total, (long long)nbytes);
    if (!is_device_ptr(stream))   // a filter byte above 4 never reaches the kernel
        for (int ps = 0; ps < g.npass; ++ps)
            for (int32_t py = 0; g.pass[ps].pw && py < g.pass[ps].ph; ++py)
                ME_CHECK(stream[g.pass[ps].offset + (int64_t)py * ((int64_t)g.pass[ps].stride + 1)] <= 4, ME_ERR_BAD_ARG,
                         "me_op_png_unfilter: bad PNG filter");
    const uint8_t* s = (const uint8_t*)to_device(ctx, stream, (size_t)nbytes, "png.op.in");
    OutBuf o = out_buf(ctx, out, (size_t)nbytes, "png.op.out");
    png_unfilter(ctx, s, (uint8_t*)o.dev, width, height, bit_depth, colour_type, interlace, band_rows);
    finish(ctx, o);
    ME_API_END(ctx)
}

// ---- the JPEG entropy leg on the device (jpeg_entropy.hip) ------------------------------------------------------------------
int32_t me_ctx_set_jpeg_entropy(me_ctx* ctx, int32_t mode) {
    ME_API_BEGIN(ctx)
    ME_CHECK(mode == 0 || mode == 1, ME_ERR_BAD_ARG, "me_ctx_set_jpeg_entropy: mode %d (0 host, 1 device)", mode);
    ctx->jpeg_entropy_mode = mode;
    ME_API_END(ctx)
}

int32_t me_last_jpeg_entropy(me_ctx* ctx, int64_t report[8], double ms[3]) {
    ME_API_BEGIN(ctx)
    ME_CHECK(report && ms, ME_ERR_BAD_ARG, "me_last_jpeg_entropy: null pointer");
    ME_CHECK(ctx->jpeg_timed || ctx->jpeg_entropy_reported, ME_ERR_NOT_READY,
             "me_last_jpeg_entropy: no JPEG decode has completed on this context");
    // a decode that never tried the device (mode 0) reports the host, with nothing else to say
    const JpegEntropyReport r = ctx->jpeg_entropy_reported ? ctx->jpeg_entropy_report : JpegEntropyReport();
    report[0] = r.where, report[1] = r.reason, report[2] = r.segments, report[3] = r.subseqs, report[4] = r.subseq_bits;
    report[5] = r.rounds, report[6] = r.upload_bytes, report[7] = r.workgroups;
    for (int i = 0; i < 3; ++i) ms[i] = r.ms[i];
    ME_API_END(ctx)
}

int32_t me_op_jpeg_entropy(me_ctx* ctx, const uint8_t* file, int64_t nbytes, int32_t subseq_bits, int16_t* coef,
                           int64_t count) {
    ME_API_BEGIN(ctx)
    ME_CHECK(file && coef && nbytes >= 0, ME_ERR_BAD_ARG, "me_op_jpeg_entropy: null pointer");
    ME_CHECK(!is_device_ptr(file), ME_ERR_BAD_ARG, "me_op_jpeg_entropy: the file's bytes must be in host memory");
    const std::vector<uint8_t> bytes(file, file + nbytes);
    matrix_eyes::JpegEntropyPlan plan;
    if (!jpeg_entropy_decode(ctx, bytes, subseq_bits, plan)) {
        ctx->last_error = "me_op_jpeg_entropy: declined, reason " + std::to_string(ctx->jpeg_entropy_report.reason) +
                          (plan.why.empty() ? "" : " (" + plan.why + ")");
        return ME_OP_JPEG_ENTROPY_DECLINED;
    }
    ME_CHECK(count == (int64_t)plan.frame.total_coefs, ME_ERR_BAD_SHAPE, "me_op_jpeg_entropy: the file has %zu coefficients, not %lld",
             plan.frame.total_coefs, (long long)count);
    from_device(ctx, coef, site_buf(ctx, "jpeg.coef", (size_t)count * sizeof(int16_t)), (size_t)count * sizeof(int16_t));
    ME_API_END(ctx)
}

int32_t me_op_jpeg_coefficients_host(const uint8_t* file, int64_t nbytes, int16_t* coef, int64_t count) {
    if (!file || nbytes < 0 || !coef) return -1;
    try {
        const std::vector<uint8_t> bytes(file, file + nbytes);
        const matrix_eyes::JpegCoefficients c = matrix_eyes::decode_jpeg_coefficients(bytes, "<jpeg>");
        if ((int64_t)c.total_coefs != count) return -2;
        std::memcpy(coef, c.comps[0].coef, (size_t)count * sizeof(int16_t));
    } catch (const std::exception&) {
        return -3;
    }
    return 0;
}

}  // extern "C"
