// Image file I/O and resampling for the C++ host layer (the reference uses the `image` and `kamadak-exif`
// crates: reconstruction.rs:96-113,133-143, output.rs:133-138,192,206-218).  Decoded here: JPEG (baseline and
// progressive Huffman, jpeg_decoder.cpp), PNG (8/16-bit, non-interlaced, zlib) and binary PPM; encoded: PNG
// and PPM.  Anything else is an ImageError, as an unsupported format is in the reference.
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace matrix_eyes {

struct ImageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

constexpr int64_t kMaxPixels = 1ll << 28;  // decoders refuse larger pictures instead of allocating for them

struct RgbImage {  // image::RgbImage: row-major, 3 bytes per pixel
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;
    RgbImage() = default;
    RgbImage(uint32_t w, uint32_t h) : width(w), height(h), data((size_t)w * h * 3) {}
};

// What the reference reads from the file besides the pixels (reconstruction.rs:97-105): the EXIF orientation
// (1..8, 1 = none) and exif::Tag::FocalLengthIn35mmFilm of the primary image.
struct ImageMetadata {
    int orientation = 1;
    std::optional<uint32_t> focal_length_35mm;
};

// ImageReader::open(..).into_decoder() + DynamicImage::from_decoder(..).into_rgb8(); the orientation is NOT
// applied here (the reference applies it as a separate step)
RgbImage load_image(const std::string& path, ImageMetadata* metadata = nullptr);
// DynamicImage::apply_orientation with the EXIF value: 2 flip horizontally, 3 rotate 180, 4 flip vertically,
// 5 rotate 90 + flip horizontally, 6 rotate 90, 7 rotate 270 + flip horizontally, 8 rotate 270 (clockwise)
RgbImage apply_orientation(const RgbImage& img, int orientation);
// the raw TIFF-structured EXIF block (after "Exif\0\0" in a JPEG APP1 segment, or a PNG eXIf chunk)
ImageMetadata parse_exif(const std::vector<uint8_t>& exif);
RgbImage decode_jpeg(const std::vector<uint8_t>& file, const std::string& path, std::vector<uint8_t>* exif);

// The JPEG decoder up to and including the entropy-coded segments (every scan type, restart intervals, interleaved or
// not): the frame and its quantised DCT coefficients, before any reconstruction.  decode_jpeg is this plus the
// reconstruction; the device decoder (csrc/jpeg_decode.hip) reconstructs from the same struct on the GPU.
struct JpegComponent {
    int id = 0, h = 1, v = 1, tq = 0;
    int width = 0, height = 0;        // samples: ceil(W * h / hmax), ceil(H * v / vmax)
    int blocks_w = 0, blocks_h = 0;   // allocated blocks (whole MCUs)
    int16_t* coef = nullptr;          // blocks_w * blocks_h * 64, natural (de-zigzagged) order, block-major
};
struct JpegCoefficients {
    int width = 0, height = 0, hmax = 1, vmax = 1;
    std::vector<JpegComponent> comps;      // 1 or 3
    uint16_t qt[4][64] = {};               // natural order
    bool qt_present[4] = {false, false, false, false};
    int adobe_transform = -1;              // -1: no Adobe marker
    size_t exif_offset = 0, exif_nbytes = 0;  // the TIFF-structured EXIF block inside the file (0, 0: none)
    size_t total_coefs = 0;                // of all components, in component order
    std::vector<int16_t> storage;          // the coefficients, unless the caller's allocator provided the memory
};
// `alloc` (optional) is called once, at the frame header, with the number of int16_t of all components together and
// returns memory for them that outlives the struct's use (pinned memory of the device path); the decoder zero-fills it
using JpegCoefAlloc = int16_t* (*)(void* user, size_t count);
JpegCoefficients decode_jpeg_coefficients(const std::vector<uint8_t>& file, const std::string& path,
                                          JpegCoefAlloc alloc = nullptr, void* alloc_user = nullptr);
// frame header and EXIF span only (no entropy decoding); comps carry no coefficients
JpegCoefficients parse_jpeg_header(const std::vector<uint8_t>& file, const std::string& path);
// the refusals of the reconstruction, in its order and with its words: an undefined quantisation table, fractional
// sampling ratios.  Throws ImageError.
void check_jpeg_reconstructible(const JpegCoefficients& c, const std::string& path);
// the 64 doubles basis[x][u] of the decoder's separable IDCT (csrc/jpeg_basis.cpp: one function for host and device)
void jpeg_idct_basis(double basis[64]);
void save_image(const RgbImage& img, const std::string& path);    // RgbImage::save: format from the extension
// DynamicImage::resize_exact(w, h, FilterType::Lanczos3); the identity when the size already matches
RgbImage resize_exact_lanczos3(const RgbImage& img, uint32_t width, uint32_t height);

}  // namespace matrix_eyes
