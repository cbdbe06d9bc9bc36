// Image file I/O and resampling for the C++ host layer (the reference uses the `image` and `kamadak-exif`
// crates: reconstruction.rs:96-113,133-143, output.rs:133-138,192,206-218).  Decoded here: JPEG (baseline and
// progressive Huffman, jpeg_decoder.cpp), PNG (every colour type and depth, Adam7; png_decoder.cpp) and binary PPM; encoded: PNG,
// baseline JPEG (jpeg_encoder.cpp) and PPM.  Anything else is an ImageError, as an unsupported format is in the reference.
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/png_recon.h"

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

// The PNG decoder (png_decoder.cpp), cut where the device decoder (csrc/png_decode.hip) takes over: the chunks, then the
// inflate, then the reconstruction.  decode_png is the three in a row; `exif` receives the last eXIf chunk's bytes.
struct PngSpan {
    size_t offset = 0, nbytes = 0;   // inside the file
};
struct PngFrame {
    uint32_t width = 0, height = 0;
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> plte;                 // the last PLTE chunk's bytes
    size_t exif_offset = 0, exif_nbytes = 0;   // the last eXIf chunk's body (0, 0: none)
    std::vector<PngSpan> idat;                 // the IDAT bodies, in file order
    size_t bits_pp = 0, bpp = 0;               // bits per pixel; the filters' byte distance
    size_t total = 0;                          // bytes of the filtered stream: (stride + 1) * ph of every pass
    me_pngdec::Geom geom;                         // the same and, per pass, x0, y0, dx, dy, pw, ph, stride and its offset
};
// every refusal of decode_png that needs no inflating, in its words and order
PngFrame parse_png_header(const std::vector<uint8_t>& file, const std::string& path);
// The IDAT data inflated (zlib's streaming inflate) into dst[frame.total]: the filtered stream, filter byte plus row, pass
// after pass.  A stream that ends short, runs long, fails its Adler-32 or is damaged throws "PNG data does not inflate to
// the image size"; bytes behind the stream's end inside IDAT are ignored.  band_cb (optional) is called with the number
// of stream bytes complete so far, every few hundred KiB: a caller can start work on the rows that are finished.
using PngBandCallback = void (*)(void* user, size_t complete);
void inflate_png(const PngFrame& frame, const std::vector<uint8_t>& file, const std::string& path, uint8_t* dst,
                 PngBandCallback band_cb = nullptr, void* band_user = nullptr);
RgbImage decode_png(const std::vector<uint8_t>& file, const std::string& path, std::vector<uint8_t>* exif);

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
// What the device entropy decoder (csrc/jpeg_entropy.h) needs of a file, and whether it may take it: parse() with the
// entropy loops skipped.  `frame` is parse_jpeg_header's struct with the FINAL quantisation tables (a DQT behind the scan
// counts, as in the host decoder, whose reconstruction runs after the whole file is parsed).  A file is eligible when the
// frame is SOF0 / SOF1, its one scan holds all frame components, every Huffman table the scan uses is a prefix code
// (Kraft sum <= 1) whose DC values are at most 15, no marker but RSTn stands inside the scan and there are as many RSTn
// as the restart interval needs; everything else (progressive files, several scans, ...) declines with a reason and is
// decoded by decode_jpeg_coefficients.  Throws ImageError where parse() does outside the entropy-coded data.
enum JpegEntropyDecline : int {
    kJpegEntropyOk = 0,
    kJpegDeclineProgressive = 1,   // SOF2
    kJpegDeclineScans = 2,         // no scan, several scans, or a scan without all frame components
    kJpegDeclineHuffman = 3,       // a table of the scan is not a prefix code (Kraft sum > 1)
    kJpegDeclineDcValue = 4,       // a DC table of the scan holds a value above 15
    kJpegDeclineMarker = 5,        // a marker other than RSTn (or a fill byte) inside the scan
    kJpegDeclineRestarts = 6,      // fewer RSTn than the restart interval needs
    kJpegDeclineLayout = 7,        // more than 10 blocks per MCU, or a scan of 2^28 bytes and more
    kJpegDeclineHostError = 8,     // the planner itself refused the file: the host decoder says why
    // at run time, through the device decoder's status word (csrc/jpeg_entropy.h)
    kJpegDeclineBadCode = 10,      // the true chain met an invalid Huffman code
    kJpegDeclineBadRun = 11,       // ... or an AC run past coefficient 63
    kJpegDeclineNoSync = 12,       // no synchronisation within the give-up distance
    kJpegDeclineShort = 13         // a segment ends before its MCUs do (the host decoder reads zeros there)
};
struct JpegHuffmanSpec {
    bool present = false;
    uint8_t counts[16] = {};       // codes of length 1..16
    uint8_t values[256] = {};
    int nvalues = 0;
};
struct JpegEntropyPlan {
    JpegCoefficients frame;        // geometry, final tables, EXIF span; comps carry no coefficients
    bool eligible = false;
    int reason = kJpegEntropyOk;   // JpegEntropyDecline
    std::string why;               // the reason in words ("progressive", ...)
    int restart_interval = 0;      // MCUs (0: none), as in force at the scan
    int mcus_x = 0, mcus_y = 0;
    int scan_comps = 0;            // components of the scan, in its order:
    int scan_comp[3] = {0, 0, 0};  //   index into frame.comps
    int scan_td[3] = {0, 0, 0}, scan_ta[3] = {0, 0, 0};
    JpegHuffmanSpec dc[4], ac[4];  // as in force at the scan
    size_t scan_begin = 0, scan_end = 0;   // the entropy-coded data: file[scan_begin, scan_end), stuffing and RSTn included
    // segment j: file[seg_begin[j], seg_end[j]) -- from behind the j-th RSTn (the scan's start for j = 0) to the first
    // marker, whatever the RSTn's numbers; only the segments the MCU count needs
    std::vector<size_t> seg_begin, seg_end;
};
JpegEntropyPlan plan_jpeg_entropy(const std::vector<uint8_t>& file, const std::string& path);
// the refusals of the reconstruction, in its order and with its words: an undefined quantisation table, fractional
// sampling ratios.  Throws ImageError.
void check_jpeg_reconstructible(const JpegCoefficients& c, const std::string& path);
// the 64 doubles basis[x][u] of the decoder's separable IDCT (csrc/jpeg_basis.cpp: one function for host and device)
void jpeg_idct_basis(double basis[64]);
void save_image(const RgbImage& img, const std::string& path);    // RgbImage::save: format from the extension
// RgbImage::save to ".jpg" / ".jpeg": a baseline JFIF file (one interleaved scan, the Annex K tables, no restart markers),
// byte for byte what libjpeg writes for the same quality (1..100) and subsampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0) with
// its integer DCT and optimize off.  Throws ImageError for parameters outside those ranges or a side above 65535.
std::vector<uint8_t> encode_jpeg(const RgbImage& img, int quality, int subsampling);
// what save_image encodes a JPEG with: MATRIX_EYES_JPEG_QUALITY (default 75) and MATRIX_EYES_JPEG_SUBSAMPLING ("4:4:4",
// "4:2:2" or "4:2:0", the default); anything else in either variable is an ImageError
struct JpegOutputParams {
    int quality = 75, subsampling = 2;
};
JpegOutputParams jpeg_output_params();
// DynamicImage::resize_exact(w, h, FilterType::Lanczos3); the identity when the size already matches
RgbImage resize_exact_lanczos3(const RgbImage& img, uint32_t width, uint32_t height);

}  // namespace matrix_eyes
