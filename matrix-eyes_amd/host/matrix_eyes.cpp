#include "matrix_eyes.hpp"

#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>

#include "matrix_eyes_hip.h"

namespace matrix_eyes {

namespace {

std::string last_error(const me_ctx* ctx) { return me_last_error(ctx); }

void check_model(const me_ctx* ctx, int32_t rc, const char* what) {
    if (rc != ME_OK) throw ModelError(rc, std::string("Model error: ") + what + ": " + last_error(ctx));
}

void check_output(const me_ctx* ctx, int32_t rc) {
    if (rc != ME_OK) throw output::OutputError(last_error(ctx));
}

bool ends_with_ci(const std::string& s, const char* suffix) {
    const size_t n = std::strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)s[s.size() - n + i]) != suffix[i]) return false;
    return true;
}

// f32::round (half away from zero) then `as u32` (saturating)
uint32_t round_u32(float x) {
    if (!(x > 0.0f)) return 0;
    const float r = std::round(x);
    return r >= 4294967296.0f ? 4294967295u : (uint32_t)r;
}

bool is_jpeg_name(const std::string& path) { return ends_with_ci(path, ".jpg") || ends_with_ci(path, ".jpeg"); }

// NAME=host | device in the environment -> whether the device does it; unset: `fallback`
bool env_host_or_device(const char* name, bool fallback) {
    const char* value = std::getenv(name);
    if (!value) return fallback;
    if (std::strcmp(value, "device") == 0) return true;
    if (std::strcmp(value, "host") != 0) throw ModelError(ME_ERR_BAD_ARG, std::string(name) + "=" + value + ": expected host or device");
    return false;
}

// MATRIX_EYES_NOISE=legacy | host | device; unset: legacy
NoiseSource env_noise_source() {
    const char* value = std::getenv("MATRIX_EYES_NOISE");
    if (!value || std::strcmp(value, "legacy") == 0) return NoiseSource::Legacy;
    if (std::strcmp(value, "host") == 0) return NoiseSource::Host;
    if (std::strcmp(value, "device") == 0) return NoiseSource::Device;
    throw ModelError(ME_ERR_BAD_ARG, std::string("MATRIX_EYES_NOISE=") + value + ": expected legacy, host or device");
}

// The key of the keyed noise: MATRIX_EYES_SEED as a full unsigned 64-bit decimal, expanded by me_noise_key_from_seed;
// unset: 32 bytes from the operating system
void noise_key(uint8_t key[32]) {
    const char* seed = std::getenv("MATRIX_EYES_SEED");
    if (!seed) {
        if (me_noise_key_from_os(key) != ME_OK) throw output::OutputError(me_last_error(nullptr));
        return;
    }
    char* end = nullptr;
    errno = 0;
    const unsigned long long v = std::strtoull(seed, &end, 10);
    if (!std::isdigit((unsigned char)seed[0]) || *end != 0 || errno == ERANGE)
        throw output::OutputError(std::string("MATRIX_EYES_SEED=") + seed + ": expected an unsigned 64-bit decimal number");
    me_noise_key_from_seed((uint64_t)v, key);
}

// save_image for the output methods: its ImageError is their OutputError
void save_or_throw(const RgbImage& image, const std::string& path) {
    try {
        save_image(image, path);
    } catch (const ImageError& err) {
        throw output::OutputError(err.what());
    }
}

void progress_trampoline(void* user, float pos, const char* message) {
    ProgressListener* pl = (ProgressListener*)user;
    pl->report_status(pos);
    if (message) pl->update_message(message);
}

}  // namespace

// ---- Device ----------------------------------------------------------------------------------------
Device::Device() {
    const char* dev = std::getenv("MATRIX_EYES_DEVICE");
    const char* dt = std::getenv("MATRIX_EYES_DTYPE");
    const char* model = std::getenv("MATRIX_EYES_MODEL");  // "tiny": the test geometry of the parity suite
    device_resampler_ = env_host_or_device("MATRIX_EYES_RESAMPLER", true);
    device_png_encoder_ = env_host_or_device("MATRIX_EYES_PNG_ENCODER", false);
    device_jpeg_decoder_ = env_host_or_device("MATRIX_EYES_JPEG_DECODER", false);
    device_png_decoder_ = env_host_or_device("MATRIX_EYES_PNG_DECODER", false);
    device_jpeg_encoder_ = env_host_or_device("MATRIX_EYES_JPEG_ENCODER", false);
    noise_source_ = env_noise_source();
    try {  // MATRIX_EYES_JPEG_QUALITY, MATRIX_EYES_JPEG_SUBSAMPLING: refused here, not at the first ".jpg" written
        jpeg_params_ = jpeg_output_params();
    } catch (const ImageError& err) {
        throw ModelError(ME_ERR_BAD_ARG, err.what());
    }
    // acts only behind MATRIX_EYES_JPEG_DECODER=device: the host decoder has one entropy loop
    const bool device_jpeg_entropy = env_host_or_device("MATRIX_EYES_JPEG_ENTROPY", false);
    // who packs the checkpoint's tensors into the weight arena (the same bytes either way)
    const bool device_weight_packer = env_host_or_device("MATRIX_EYES_WEIGHT_PACKER", false);
    me_model_config cfg;
    me_default_config(&cfg);
    if (model && std::strcmp(model, "tiny") == 0) {
        cfg.grid = 8, cfg.embed_dim = 128, cfg.num_heads = 2, cfg.depth = 4;
        cfg.tap_blocks[0] = 1, cfg.tap_blocks[1] = 2;
        cfg.enc_dims[0] = 64, cfg.enc_dims[1] = cfg.enc_dims[2] = cfg.enc_dims[3] = 128;
        cfg.dec_dim = 256, cfg.head_dims[0] = 32, cfg.head_dims[1] = 1;
    }
    image_size_ = 64 * cfg.grid;
    const int32_t dtype = dt && std::strcmp(dt, "bf16") == 0 ? ME_DTYPE_BF16 : (dt && std::strcmp(dt, "fp8") == 0 ? ME_DTYPE_FP8 : ME_DTYPE_F16);
    const int32_t rc = me_ctx_create(dev ? std::atoi(dev) : 0, dtype,
                                     &cfg, &ctx_);
    if (rc != ME_OK) throw ModelError(rc, std::string("cannot initialise the HIP device: ") + me_last_error(nullptr));
    if (device_jpeg_entropy && me_ctx_set_jpeg_entropy(ctx_, 1) != ME_OK) throw ModelError(ME_ERR_BAD_ARG, me_last_error(ctx_));
    if (device_weight_packer && me_ctx_set_weight_packer(ctx_, 1) != ME_OK) throw ModelError(ME_ERR_BAD_ARG, me_last_error(ctx_));
}

Device::~Device() {
    if (ctx_) me_ctx_destroy(ctx_);
}

void Device::set_write_behind(int files_in_flight) const {
    if (me_ctx_set_write_behind(ctx_, files_in_flight) != ME_OK) throw output::OutputError(me_last_error(ctx_));
}

void Device::flush_outputs() const {
    if (me_output_flush(ctx_) != ME_OK) throw output::OutputError(me_last_error(ctx_));  // OutputError::Io of a file written behind
}

RgbImage Device::resize_exact_lanczos3(const RgbImage& img, uint32_t width, uint32_t height) const {
    if (!device_resampler_) return matrix_eyes::resize_exact_lanczos3(img, width, height);
    if (img.width == 0 || img.height == 0 || width == 0 || height == 0 || img.width > (uint32_t)ME_RESIZE_MAX_DIM ||
        img.height > (uint32_t)ME_RESIZE_MAX_DIM || width > (uint32_t)ME_RESIZE_MAX_DIM || height > (uint32_t)ME_RESIZE_MAX_DIM)
        throw ImageError("cannot resize " + std::to_string(img.width) + "x" + std::to_string(img.height) + " to " +
                         std::to_string(width) + "x" + std::to_string(height));
    RgbImage out(width, height);
    const int32_t rc = me_resize_lanczos3_rgb8(ctx_, img.data.data(), (int32_t)img.width, (int32_t)img.height, out.data.data(),
                                               (int32_t)width, (int32_t)height);
    if (rc != ME_OK) throw ImageError(std::string("cannot resize: ") + me_last_error(ctx_));
    return out;
}

bool Device::load_decoded_resized(const std::string& path, bool with_orientation, uint32_t width, uint32_t height, RgbImage* out,
                                  ImageMetadata* metadata, uint32_t* original_width, uint32_t* original_height) const {
    const bool jpeg_name = ends_with_ci(path, ".jpg") || ends_with_ci(path, ".jpeg"), png_name = ends_with_ci(path, ".png");
    if (!(device_jpeg_decoder_ && jpeg_name) && !(device_png_decoder_ && png_name)) return false;
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ImageError("cannot open " + path);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    // load_image goes by the signature
    static const uint8_t kPngSig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    const bool png = file.size() >= 8 && !std::memcmp(file.data(), kPngSig, 8);
    const bool jpeg = !png && file.size() >= 3 && file[0] == 0xff && file[1] == 0xd8 && file[2] == 0xff;
    if (!(jpeg && jpeg_name) && !(png && png_name)) return false;
    // the library says "<jpeg>: ..." / "<png>: ..." where the host decoder says "<path>: ..."
    const std::string tag = png ? "<png>" : "<jpeg>";
    auto refuse = [&](const char* message) {
        const std::string m = message ? message : "";
        throw ImageError(m.rfind(tag, 0) == 0 ? path + m.substr(tag.size()) : m);
    };
    const auto info = png ? me_png_info : me_jpeg_info;
    const auto decode = png ? me_png_decode_rgb8 : me_jpeg_decode_rgb8;
    const auto decode_resized = png ? me_png_decode_resized_rgb8 : me_jpeg_decode_resized_rgb8;
    int32_t w = 0, h = 0;
    int64_t exif_offset = 0, exif_nbytes = 0;
    if (info(file.data(), (int64_t)file.size(), &w, &h, &exif_offset, &exif_nbytes) != ME_OK) refuse(me_last_error(nullptr));
    const ImageMetadata meta = parse_exif(std::vector<uint8_t>(file.begin() + exif_offset, file.begin() + exif_offset + exif_nbytes));
    if (metadata) *metadata = meta;
    // apply_orientation leaves the picture alone for a value outside 2..8
    const int orientation = with_orientation && meta.orientation >= 2 && meta.orientation <= 8 ? meta.orientation : 1;
    const uint32_t ow = orientation >= 5 ? (uint32_t)h : (uint32_t)w, oh = orientation >= 5 ? (uint32_t)w : (uint32_t)h;
    if (original_width) *original_width = ow;
    if (original_height) *original_height = oh;
    if (device_resampler_) {  // decode, orientation and resize chained on the GPU: only the resized picture comes back
        *out = RgbImage(width, height);
        const int32_t rc = decode_resized(ctx_, file.data(), (int64_t)file.size(), orientation, out->data.data(), (int32_t)width,
                                          (int32_t)height);
        if (rc != ME_OK) refuse(me_last_error(ctx_));
        return true;
    }
    RgbImage full(ow, oh);
    const int32_t rc = decode(ctx_, file.data(), (int64_t)file.size(), orientation, full.data.data(), (int32_t)ow, (int32_t)oh);
    if (rc != ME_OK) refuse(me_last_error(ctx_));
    *out = matrix_eyes::resize_exact_lanczos3(full, width, height);
    return true;
}

// ---- DepthProModelLoader -----------------------------------------------------------------------------
void DepthProModelLoader::ensure_loaded(const Device& device) const {
    if (device.weights_loaded_) return;
    me_ctx* ctx = device.ctx();
    // mod.rs:211-249: a valid arena cache beside the checkpoint is loaded instead of it; otherwise the library reads the
    // PyTorch archive itself (keys the model does not use are skipped) and, with --convert-checkpoints, writes the cache
    const int32_t rc = me_load_checkpoint_cached(ctx, checkpoint_path_.c_str(), convert_checkpoints_ ? 1 : 0, nullptr);
    if (rc == ME_ERR_IO)  // LoaderError::Pytorch
        throw ModelError(ME_ERR_IO, std::string("Model error: ") + me_last_error(ctx));
    check_model(ctx, rc, "failed to load checkpoint");
    device.weights_loaded_ = true;
}

std::vector<float> DepthProModelLoader::extract_depth(const Device& device, const RgbImage& img,
                                                      std::optional<float> f_norm, ProgressListener* pl) const {
    const int S = device.image_size();
    if ((int)img.width != S || (int)img.height != S)
        throw ModelError(ME_ERR_BAD_SHAPE, "Model error: image is not " + std::to_string(S) + "x" + std::to_string(S));
    ensure_loaded(device);
    me_ctx* ctx = device.ctx();
    me_ctx_set_progress(ctx, pl ? progress_trampoline : nullptr, pl);
    std::vector<float> depth((size_t)S * S);
    const float fn = f_norm.value_or(0.f);
    const int32_t rc = me_extract_depth_u8(ctx, img.data.data(), 1, f_norm ? &fn : nullptr, depth.data(), nullptr);
    me_ctx_set_progress(ctx, nullptr, nullptr);
    check_model(ctx, rc, "failed to run the model");
    return depth;
}

// ---- output::DepthMap --------------------------------------------------------------------------------
namespace output {

DepthMap::DepthMap(const Device& device, std::vector<float> inverse_depth, size_t rows, size_t cols,
                   uint32_t original_width, uint32_t original_height)
    : device_(device), data_(std::move(inverse_depth)), data_width_(rows), data_height_(cols),
      original_width_(original_width), original_height_(original_height) {
    if (data_.size() != rows * cols) throw OutputError("DepthMap: data does not match its dimensions");
    check_output(device_.ctx(), me_depth_clamp_minmax(device_.ctx(), data_.data(), (int64_t)data_.size(), &min_, &max_));
}

void DepthMap::output_image(const std::string& destination_path, const std::string& source_path,
                            ImageOutputFormat image_format, VertexMode vertex_mode) const {
    if (ends_with_ci(destination_path, ".ply") || ends_with_ci(destination_path, ".obj") || ends_with_ci(destination_path, ".glb"))
        return output_mesh(destination_path, source_path, vertex_mode);
    if (image_format.kind == ImageOutputFormat::DepthMap) return output_depth_map(destination_path);
    return output_stereogram(destination_path, image_format.resize_scale, image_format.amplitude);
}

void DepthMap::output_depth_map(const std::string& destination_path) const {
    if (device_.device_resampler() && device_.device_png_encoder() && ends_with_ci(destination_path, ".png")) {
        // ... and the save: filtered and compressed on the GPU, only the file's bytes come back
        check_output(device_.ctx(), me_output_depth_map_png(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_,
                                                            min_, max_, nullptr, (int32_t)original_width_, (int32_t)original_height_,
                                                            destination_path.c_str()));
        return;
    }
    if (device_.device_resampler() && device_.device_jpeg_encoder() && is_jpeg_name(destination_path)) {
        // ... or, to a ".jpg": transformed, Huffman-coded and stuffed on the GPU
        const JpegOutputParams& p = device_.jpeg_params();
        check_output(device_.ctx(), me_output_depth_map_jpeg(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_,
                                                             min_, max_, nullptr, (int32_t)original_width_, (int32_t)original_height_,
                                                             p.quality, p.subsampling, destination_path.c_str()));
        return;
    }
    if (device_.device_resampler()) {  // the colour map and the resize chained on the GPU
        RgbImage resized(original_width_, original_height_);
        check_output(device_.ctx(), me_depthmap_rgb_resized(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_, min_,
                                                            max_, nullptr, (int32_t)original_width_, (int32_t)original_height_,
                                                            resized.data.data()));
        return save_or_throw(resized, destination_path);
    }
    RgbImage out((uint32_t)data_width_, (uint32_t)data_height_);
    check_output(device_.ctx(), me_depthmap_rgb(device_.ctx(), data_.data(), (int64_t)data_.size(), min_, max_, out.data.data()));
    try {
        save_image(resize_exact_lanczos3(out, original_width_, original_height_), destination_path);
    } catch (const ImageError& err) {
        throw OutputError(err.what());
    }
}

void DepthMap::output_stereogram(const std::string& destination_path, std::optional<float> resize_scale,
                                 float amplitude) const {
    uint32_t w = original_width_, h = original_height_;
    if (resize_scale) {  // output.rs:147-151, f32 arithmetic
        w = round_u32((float)original_width_ * *resize_scale);
        h = round_u32((float)original_height_ * *resize_scale);
    }
    const bool to_png = device_.device_png_encoder() && ends_with_ci(destination_path, ".png");
    const bool to_jpeg = device_.device_jpeg_encoder() && is_jpeg_name(destination_path);
    if (device_.noise_source() == NoiseSource::Device) {
        // the keyed entries: the noise is made on the GPU, in device scratch; no noise buffer exists here
        uint8_t key[32];
        noise_key(key);
        if (to_png) {
            check_output(device_.ctx(), me_output_stereogram_png_keyed(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_,
                                                                       min_, max_, (int32_t)w, (int32_t)h, amplitude, key, destination_path.c_str()));
            return;
        }
        if (to_jpeg) {
            const JpegOutputParams& p = device_.jpeg_params();
            check_output(device_.ctx(), me_output_stereogram_jpeg_keyed(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_,
                                                                        min_, max_, (int32_t)w, (int32_t)h, amplitude, key, p.quality,
                                                                        p.subsampling, destination_path.c_str()));
            return;
        }
        RgbImage out(w, h);
        check_output(device_.ctx(), me_stereogram_keyed(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_, min_, max_,
                                                        (int32_t)w, (int32_t)h, amplitude, key, out.data.data()));
        return save_or_throw(out, destination_path);
    }
    RgbImage noise(w, h), out(w, h);
    if (device_.noise_source() == NoiseSource::Host) {
        // the same bytes from the CPU twin, on this thread
        uint8_t key[32];
        noise_key(key);
        if (me_stereogram_noise_host(key, (int32_t)w, (int32_t)h, noise.data.data()) != ME_OK) throw OutputError(me_last_error(nullptr));
    } else {
        // output.rs:165-171: rand::rng() fills one [u8; 3] per pixel, row by row.  MATRIX_EYES_SEED makes a
        // run repeatable (the reference is not).
        const char* seed = std::getenv("MATRIX_EYES_SEED");
        std::mt19937 rng(seed ? (unsigned)std::strtoul(seed, nullptr, 10) : std::random_device{}());
        for (size_t i = 0; i < noise.data.size(); i += 4) {
            const uint32_t v = rng();
            for (size_t k = 0; k < 4 && i + k < noise.data.size(); ++k) noise.data[i + k] = (uint8_t)(v >> (8 * k));
        }
    }
    if (device_.device_png_encoder() && ends_with_ci(destination_path, ".png")) {
        check_output(device_.ctx(), me_output_stereogram_png(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_,
                                                             min_, max_, (int32_t)w, (int32_t)h, amplitude, noise.data.data(),
                                                             destination_path.c_str()));
        return;
    }
    if (device_.device_jpeg_encoder() && is_jpeg_name(destination_path)) {
        const JpegOutputParams& p = device_.jpeg_params();
        check_output(device_.ctx(), me_output_stereogram_jpeg(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_,
                                                              min_, max_, (int32_t)w, (int32_t)h, amplitude, noise.data.data(),
                                                              p.quality, p.subsampling, destination_path.c_str()));
        return;
    }
    check_output(device_.ctx(), me_stereogram(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_, min_, max_,
                                              (int32_t)w, (int32_t)h, amplitude, noise.data.data(), out.data.data()));
    save_or_throw(out, destination_path);
}

void DepthMap::output_mesh(const std::string& destination_path, const std::string& source_path, VertexMode mode) const {
    std::vector<uint8_t> colors;
    if (mode == VertexMode::Color) {  // output.rs:206-218
        try {
            RgbImage resized;  // the source as decoded (no orientation), resized to the depth map
            if (!device_.load_decoded_resized(source_path, false, (uint32_t)data_width_, (uint32_t)data_height_, &resized, nullptr,
                                              nullptr, nullptr))
                resized = device_.resize_exact_lanczos3(load_image(source_path), (uint32_t)data_width_, (uint32_t)data_height_);
            colors = std::move(resized.data);
        } catch (const ImageError& err) {
            throw OutputError(err.what());
        }
    }
    check_output(device_.ctx(),
                 me_output_mesh(device_.ctx(), data_.data(), (int32_t)data_width_, (int32_t)data_height_, original_width_,
                                original_height_, destination_path.c_str(), source_path.c_str(),
                                mode == VertexMode::Plain ? ME_VERTEX_PLAIN : (mode == VertexMode::Color ? ME_VERTEX_COLOR : ME_VERTEX_TEXTURE),
                                colors.empty() ? nullptr : colors.data()));
}

}  // namespace output

// ---- reconstruction ------------------------------------------------------------------------------------
namespace reconstruction {

namespace {

// indicatif's bar in the reference (reconstruction.rs:207-238); a single rewritten line here
struct ProgressReporter : ProgressListener {
    std::string message;
    void report_status(float pos) override {
        std::fprintf(stderr, "\r[%3d%%]%s\033[K", (int)std::lround(pos * 100.0f), message.c_str());
        std::fflush(stderr);
    }
    void update_message(const std::string& status_message) override { message = ": " + status_message; }
    ~ProgressReporter() override { std::fprintf(stderr, "\r\033[K"); }
};

}  // namespace

SourceImage SourceImage::load(const std::string& path, std::optional<float> focal_length_35mm, int size) {
    return load_with(nullptr, path, focal_length_35mm, size);
}

SourceImage SourceImage::load(const Device& device, const std::string& path, std::optional<float> focal_length_35mm, int size) {
    return load_with(&device, path, focal_length_35mm, size);
}

SourceImage SourceImage::load_with(const Device* device, const std::string& path, std::optional<float> focal_length_35mm, int size) {
    SourceImage s;
    RgbImage img;
    ImageMetadata meta;
    try {
        // a JPEG / PNG photo with MATRIX_EYES_JPEG_DECODER / _PNG_DECODER=device: reconstruction, orientation (:104-106) and the resize (:107-113) on the GPU
        uint32_t ow = 0, oh = 0;
        if (device && device->load_decoded_resized(path, true, (uint32_t)size, (uint32_t)size, &s.img, &meta, &ow, &oh)) {
            s.focal_length_35mm = focal_length_35mm;
            if (!s.focal_length_35mm && meta.focal_length_35mm) s.focal_length_35mm = (float)*meta.focal_length_35mm;
            s.original_width = ow, s.original_height = oh;
            return s;
        }
        img = load_image(path, &meta);
    } catch (const ImageError& err) {
        throw ReconstructionError(std::string("Image error: ") + err.what());
    }
    // reconstruction.rs:97-103: the caller's focal length wins, else EXIF FocalLengthIn35mmFilm, else none
    s.focal_length_35mm = focal_length_35mm;
    if (!s.focal_length_35mm && meta.focal_length_35mm) s.focal_length_35mm = (float)*meta.focal_length_35mm;
    img = apply_orientation(img, meta.orientation);  // :104-106
    s.original_width = img.width, s.original_height = img.height;
    try {
        s.img = device ? device->resize_exact_lanczos3(img, (uint32_t)size, (uint32_t)size)
                       : resize_exact_lanczos3(img, (uint32_t)size, (uint32_t)size);
    } catch (const ImageError& err) {
        throw ReconstructionError(std::string("Image error: ") + err.what());
    }
    return s;
}

std::optional<double> SourceImage::focal_length_px() const {
    if (!focal_length_35mm) return std::nullopt;
    const double diagonal_35mm = std::sqrt(24.0 * 24.0 + 36.0 * 36.0);
    const double w = original_width, h = original_height;
    return (double)*focal_length_35mm * std::sqrt(w * w + h * h) / diagonal_35mm;
}

void extract_depth(const Device& device, const DepthProModelLoader& model_loader, const std::string& source_path,
                   const std::string& destination_path, std::optional<float> focal_length_35mm,
                   output::ImageOutputFormat image_format, output::VertexMode vertex_mode) {
    SourceImage img;
    try {
        img = SourceImage::load(device, source_path, focal_length_35mm, device.image_size());
    } catch (const ReconstructionError& err) {
        std::fprintf(stderr, "Failed to load source image: %s\n", err.what());
        throw;
    }
    std::optional<float> f_norm;
    if (const std::optional<double> f_px = img.focal_length_px()) f_norm = (float)(*f_px / (double)img.original_width);  // :174-176
    std::vector<float> inverse_depth;
    try {
        ProgressReporter pl;
        inverse_depth = model_loader.extract_depth(device, img.img, f_norm, &pl);
    } catch (const ModelError& err) {
        std::fprintf(stderr, "Failed to process image: %s\n", err.what());
        throw ReconstructionError(err.what());
    }
    try {
        const size_t S = (size_t)device.image_size();
        const output::DepthMap depth_map(device, std::move(inverse_depth), S, S, img.original_width, img.original_height);
        depth_map.output_image(destination_path, source_path, image_format, vertex_mode);
    } catch (const output::OutputError& err) {
        std::fprintf(stderr, "Failed to output result: %s\n", err.what());
        throw ReconstructionError(std::string("Output error: ") + err.what());
    }
}

}  // namespace reconstruction

}  // namespace matrix_eyes
