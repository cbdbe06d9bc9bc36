// C++ host layer above the C ABI of include/matrix_eyes_hip.h: the reference's Rust surface for the hot
// path, type for type, so that main.cpp reads like the reference's main.rs.  (No Rust toolchain exists in
// the build image; the Rust binding itself is sketched in INTEGRATION.md.)
//
//   reference                                             here
//   reconstruction::init_device()           (:42-72)      Device
//   depth_pro::DepthProModelLoader::new     (mod.rs:167)  DepthProModelLoader(path, convert)
//   DepthProModelLoader::extract_depth      (mod.rs:251)  DepthProModelLoader::extract_depth
//   depth_pro::ProgressListener             (mod.rs:366)  ProgressListener
//   depth_pro::ModelError / LoaderError     (mod.rs:430-)  ModelError
//   output::{ImageOutputFormat, VertexMode} (:27-38)      output::ImageOutputFormat, output::VertexMode
//   output::DepthMap::{new, output_image}   (:44,100)     output::DepthMap
//   output::OutputError                     (:716-)       output::OutputError
//   reconstruction::extract_depth           (:155-205)    reconstruction::extract_depth
//   reconstruction::ReconstructionError     (:240-)       reconstruction::ReconstructionError
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "image_io.hpp"

struct me_ctx;

namespace matrix_eyes {

constexpr int IMG_SIZE = 1536;  // depth_pro::IMG_SIZE

// depth_pro::ModelError::Internal(msg, LoaderError): "Model error: {msg}: {err}"
struct ModelError : std::runtime_error {
    int code;  // the C ABI status (ME_ERR_*)
    ModelError(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

struct ProgressListener {  // mod.rs:366-372
    virtual ~ProgressListener() = default;
    virtual void report_status(float pos) = 0;
    virtual void update_message(const std::string& status_message) = 0;
};

// reconstruction::init_device(): the MI355X back end has one kind of device; MATRIX_EYES_DEVICE picks the
// GPU ordinal, MATRIX_EYES_DTYPE=bf16 the MFMA operand type (default f16: the fp16 checkpoint bit for bit).
// Where output_stereogram's noise comes from (MATRIX_EYES_NOISE): Legacy (the default) is std::mt19937 seeded with
// MATRIX_EYES_SEED or the OS, today's bytes; Host is the keyed ChaCha12 noise of DESIGN.md §4.41 made by its CPU twin
// (me_stereogram_noise_host) and handed to today's calls; Device is the same noise made on the GPU by a fill
// kernel (me_stereogram_keyed and its file forms), with no noise buffer on the host.  Host and Device write the same
// pixels for the same MATRIX_EYES_SEED (a full unsigned 64-bit decimal; unset: a key from the OS), and so does the
// Python mirror.  Any other value fails the Device constructor.
enum class NoiseSource { Legacy, Host, Device };

class Device {
public:
    Device();
    ~Device();
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    me_ctx* ctx() const { return ctx_; }
    int image_size() const { return image_size_; }  // IMG_SIZE unless a test model is selected
    // a caller that writes one mesh per image of a batch: .obj files written behind it by up to `files_in_flight` host
    // threads (me_ctx_set_write_behind); flush_outputs() before the files are read -- a failed write surfaces there
    void set_write_behind(int files_in_flight) const;
    void flush_outputs() const;
    // DynamicImage::resize_exact(width, height, FilterType::Lanczos3) (reconstruction.rs:107-113, output.rs:133-137,
    // 206-218) on the GPU (me_resize_lanczos3_rgb8) -- or, with MATRIX_EYES_RESAMPLER=host, image_io's loop on one CPU
    // core.  Both write the `image` crate's bytes; any other value of the variable fails the constructor.
    bool device_resampler() const { return device_resampler_; }
    RgbImage resize_exact_lanczos3(const RgbImage& img, uint32_t width, uint32_t height) const;
    // RgbImage::save to ".png" (output.rs:138, :192): with MATRIX_EYES_PNG_ENCODER=device output_depth_map and
    // output_stereogram make, filter and compress the picture on the GPU in one call (me_output_depth_map_png,
    // me_output_stereogram_png) and only the file's bytes come back; "host" (the default) is image_io's encode_png.  Any
    // other value fails the constructor.  The files differ in their bytes, not in their pixels.
    bool device_png_encoder() const { return device_png_encoder_; }
    // RgbImage::save to ".jpg" / ".jpeg": with MATRIX_EYES_JPEG_ENCODER=device output_depth_map and output_stereogram make
    // and encode the picture on the GPU in one call (me_output_depth_map_jpeg, me_output_stereogram_jpeg); "host" (the
    // default) is image_io's encode_jpeg.  Both write the same bytes, with MATRIX_EYES_JPEG_QUALITY (75) and
    // MATRIX_EYES_JPEG_SUBSAMPLING ("4:2:0"); any other value of the three variables fails the constructor.
    bool device_jpeg_encoder() const { return device_jpeg_encoder_; }
    const JpegOutputParams& jpeg_params() const { return jpeg_params_; }
    NoiseSource noise_source() const { return noise_source_; }
    // ImageReader::open(..).decode() of a JPEG photo (reconstruction.rs:95-106): with MATRIX_EYES_JPEG_DECODER=device the
    // entropy-coded segments are decoded on the host and the picture is reconstructed and oriented on the GPU
    // (me_jpeg_decode_rgb8), chained there with the resize when the device resampler is on (me_jpeg_decode_resized_rgb8:
    // the full-size picture never exists on the host); "host" (the default) is jpeg_decoder.cpp.  Both write the same
    // bytes; any other value fails the constructor.
    bool device_jpeg_decoder() const { return device_jpeg_decoder_; }
    // ImageReader::open(..).decode() of a PNG photo or vertex-colour source (reconstruction.rs:95-106, output.rs:206-218):
    // with MATRIX_EYES_PNG_DECODER=device zlib's inflate stays on the host and the scanline filters, the conversion to RGB,
    // the de-interlacing and the orientation run on the GPU (me_png_decode_rgb8), chained there with the resize when the
    // device resampler is on (me_png_decode_resized_rgb8); "host" (the default) is png_decoder.cpp.  Both write the same
    // bytes; any other value fails the constructor.
    bool device_png_decoder() const { return device_png_decoder_; }
    // load_image + (with_orientation: apply_orientation with the file's EXIF value) + resize_exact_lanczos3(width, height)
    // of a ".jpg" / ".jpeg" or ".png" file through its device decoder.  False (nothing done) when that decoder is "host" or
    // the file is not of the format by name and signature: the caller takes the host path.  original_*: the oriented size
    // before the resize.
    bool load_decoded_resized(const std::string& path, bool with_orientation, uint32_t width, uint32_t height, RgbImage* out,
                           ImageMetadata* metadata, uint32_t* original_width, uint32_t* original_height) const;

private:
    me_ctx* ctx_ = nullptr;
    int image_size_ = IMG_SIZE;
    bool device_resampler_ = true;
    bool device_png_encoder_ = false;
    bool device_jpeg_encoder_ = false;
    JpegOutputParams jpeg_params_;
    NoiseSource noise_source_ = NoiseSource::Legacy;
    bool device_jpeg_decoder_ = false;
    bool device_png_decoder_ = false;
    mutable bool weights_loaded_ = false;
    friend class DepthProModelLoader;
};

class DepthProModelLoader {
public:
    // convert_checkpoints: the reference caches a converted file next to the checkpoint and loads it on later runs
    // (mod.rs:211-247); here that file is the packed weight arena (me_load_checkpoint_cached: "<stem>-<dtype>-<layout
    // hash>.mearena", loaded whenever it is there and valid, written after loading when the flag is set).
    // MATRIX_EYES_WEIGHT_PACKER=host|device: who packs the .pt's tensors when there is no cache (the same arena bytes).
    DepthProModelLoader(const std::string& checkpoint_path, bool convert_checkpoints)
        : checkpoint_path_(checkpoint_path), convert_checkpoints_(convert_checkpoints) {}

    // img: RGB8 [size x size] (the normalise / permute of reconstruction.rs:116-124 happens on the GPU);
    // returns the inverse depth [size*size], clamped to [1e-4, 1e4] (mod.rs:340-362)
    std::vector<float> extract_depth(const Device& device, const RgbImage& img, std::optional<float> f_norm,
                                     ProgressListener* pl) const;

private:
    void ensure_loaded(const Device& device) const;
    std::string checkpoint_path_;
    bool convert_checkpoints_;
};

namespace output {

enum class VertexMode { Plain, Color, Texture };  // output.rs:33-38

struct ImageOutputFormat {  // output.rs:27-31
    enum Kind { DepthMap, Stereogram } kind = DepthMap;
    std::optional<float> resize_scale;  // Stereogram(resize_scale, amplitude)
    float amplitude = 1.0f / 16.0f;
    static ImageOutputFormat depth_map() { return ImageOutputFormat{}; }
    static ImageOutputFormat stereogram(std::optional<float> resize_scale, float amplitude) {
        ImageOutputFormat f;
        f.kind = Stereogram, f.resize_scale = resize_scale, f.amplitude = amplitude;
        return f;
    }
};

struct OutputError : std::runtime_error {  // output.rs:716-
    using std::runtime_error::runtime_error;
};

class DepthMap {
public:
    // DepthMap::new (output.rs:44-67): inverse_depth [rows x cols], clamped to [1/250, 1/0.1]
    DepthMap(const Device& device, std::vector<float> inverse_depth, size_t rows, size_t cols,
             uint32_t original_width, uint32_t original_height);
    std::pair<float, float> inverse_depth_range() const { return {min_, max_}; }  // :69-75
    // output.rs:100-121: .ply / .obj (and .glb, a glTF 2.0 binary mesh) by suffix, else the image format
    void output_image(const std::string& destination_path, const std::string& source_path,
                      ImageOutputFormat image_format, VertexMode vertex_mode) const;

private:
    void output_depth_map(const std::string& destination_path) const;                        // :123-139
    void output_stereogram(const std::string& destination_path, std::optional<float> resize_scale,
                           float amplitude) const;                                          // :141-193
    void output_mesh(const std::string& destination_path, const std::string& source_path,
                     VertexMode mode) const;                                                // :195-261
    const Device& device_;
    std::vector<float> data_;
    size_t data_width_, data_height_;  // names as in the reference (rows, cols of the tensor)
    uint32_t original_width_, original_height_;
    float min_ = 0.f, max_ = 0.f;
};

}  // namespace output

namespace reconstruction {

struct ReconstructionError : std::runtime_error {  // reconstruction.rs:240-249
    using std::runtime_error::runtime_error;
};

struct SourceImage {  // reconstruction.rs:74-81
    RgbImage img;                              // size x size
    uint32_t original_width = 0, original_height = 0;
    std::optional<float> focal_length_35mm;
    static SourceImage load(const std::string& path, std::optional<float> focal_length_35mm, int size);  // :87-131
    // the same with the resize made by `device` (Device::resize_exact_lanczos3)
    static SourceImage load(const Device& device, const std::string& path, std::optional<float> focal_length_35mm, int size);
    std::optional<double> focal_length_px() const;                                                       // :145-152

private:
    static SourceImage load_with(const Device* device, const std::string& path, std::optional<float> focal_length_35mm, int size);
};

// reconstruction.rs:155-205
void extract_depth(const Device& device, const DepthProModelLoader& model_loader, const std::string& source_path,
                   const std::string& destination_path, std::optional<float> focal_length_35mm,
                   output::ImageOutputFormat image_format, output::VertexMode vertex_mode);

}  // namespace reconstruction

}  // namespace matrix_eyes
