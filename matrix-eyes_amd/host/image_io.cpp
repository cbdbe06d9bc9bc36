#include "image_io.hpp"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

namespace matrix_eyes {

namespace {

std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ImageError("cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

bool ends_with_ci(const std::string& s, const char* suffix) {
    const size_t n = std::strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)s[s.size() - n + i]) != suffix[i]) return false;
    return true;
}

// ---- PNG (the decoder: png_decoder.cpp) -------------------------------------------------------------------------------------------
const uint8_t kPngSig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

void put_be32(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back(x >> 24), v.push_back(x >> 16), v.push_back(x >> 8), v.push_back(x);
}

void put_chunk(std::vector<uint8_t>& out, const char* type, const std::vector<uint8_t>& body) {
    put_be32(out, (uint32_t)body.size());
    const size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), body.begin(), body.end());
    put_be32(out, (uint32_t)crc32(0, &out[start], (uInt)(out.size() - start)));
}

void encode_png(const RgbImage& img, const std::string& path) {
    std::vector<uint8_t> out(kPngSig, kPngSig + 8), ihdr;
    put_be32(ihdr, img.width), put_be32(ihdr, img.height);
    ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});  // 8-bit RGB, no interlace
    put_chunk(out, "IHDR", ihdr);
    const size_t stride = (size_t)img.width * 3;
    std::vector<uint8_t> raw((stride + 1) * img.height);
    for (uint32_t y = 0; y < img.height; ++y) {  // filter 0: the payload is noise or a smooth colour ramp
        raw[y * (stride + 1)] = 0;
        std::memcpy(&raw[y * (stride + 1) + 1], &img.data[y * stride], stride);
    }
    uLongf clen = compressBound((uLong)raw.size());
    std::vector<uint8_t> comp(clen);
    if (compress2(comp.data(), &clen, raw.data(), (uLong)raw.size(), 6) != Z_OK) throw ImageError("zlib failed");
    comp.resize(clen);
    put_chunk(out, "IDAT", comp);
    put_chunk(out, "IEND", {});
    std::ofstream f(path, std::ios::binary);
    if (!f.write((const char*)out.data(), (std::streamsize)out.size())) throw ImageError("cannot write " + path);
}

// ---- PPM (P6) --------------------------------------------------------------------------------------
RgbImage decode_ppm(const std::vector<uint8_t>& file, const std::string& path) {
    size_t pos = 2;
    auto next_int = [&]() -> long {
        for (;;) {
            while (pos < file.size() && std::isspace(file[pos])) ++pos;
            if (pos < file.size() && file[pos] == '#') {
                while (pos < file.size() && file[pos] != '\n') ++pos;
                continue;
            }
            break;
        }
        long v = 0;
        bool any = false;
        while (pos < file.size() && std::isdigit(file[pos])) v = v * 10 + (file[pos++] - '0'), any = true;
        if (!any) throw ImageError(path + ": bad PPM header");
        return v;
    };
    const long w = next_int(), h = next_int(), maxv = next_int();
    ++pos;  // the single whitespace byte after maxval
    if (w <= 0 || h <= 0 || maxv != 255) throw ImageError(path + ": only 8-bit PPM is supported");
    if ((int64_t)w * h > kMaxPixels) throw ImageError(path + ": PPM larger than 2^28 pixels");
    RgbImage img((uint32_t)w, (uint32_t)h);
    if (pos + img.data.size() > file.size()) throw ImageError(path + ": truncated PPM");
    std::memcpy(img.data.data(), &file[pos], img.data.size());
    return img;
}

// ---- Lanczos3 --------------------------------------------------------------------------------------
float sinc(float t) {
    if (t == 0.0f) return 1.0f;
    const float a = t * 3.14159265358979323846f;
    return std::sin(a) / a;
}
float lanczos3(float x) { return std::fabs(x) < 3.0f ? sinc(x) * sinc(x / 3.0f) : 0.0f; }

// One separable pass over `len_in` samples per line; layout given by (pixel stride, line stride).
// Follows the image crate's sampler: kernel scaled by max(ratio, 1), support 3, weights renormalised,
// f32 accumulation, clamp and round on output.
void resample(const std::vector<float>& in, std::vector<float>& out, uint32_t len_in, uint32_t len_out,
              uint32_t lines, size_t in_px, size_t in_line, size_t out_px, size_t out_line) {
    const float ratio = (float)len_in / (float)len_out, sratio = ratio < 1.0f ? 1.0f : ratio;
    const float support = 3.0f * sratio;
    std::vector<float> w;
    for (uint32_t o = 0; o < len_out; ++o) {
        const float center = ((float)o + 0.5f) * ratio;
        long left = (long)std::floor(center - support), right = (long)std::ceil(center + support);
        left = std::max(0l, std::min<long>(left, (long)len_in - 1));
        right = std::max(left + 1, std::min<long>(right, (long)len_in));
        w.assign((size_t)(right - left), 0.0f);
        float sum = 0.0f;
        for (long i = left; i < right; ++i) sum += (w[(size_t)(i - left)] = lanczos3(((float)i - (center - 0.5f)) / sratio));
        for (float& v : w) v /= sum;
        for (uint32_t l = 0; l < lines; ++l)
            for (int c = 0; c < 3; ++c) {
                float acc = 0.0f;
                for (long i = left; i < right; ++i) acc += in[l * in_line + (size_t)i * in_px + c] * w[(size_t)(i - left)];
                out[l * out_line + o * out_px + c] = acc;
            }
    }
}

}  // namespace

// ---- EXIF ---------------------------------------------------------------------------------------------
// TIFF structure: byte order mark, offset of IFD0; 12-byte entries (tag, type, count, value / offset).
// Orientation (0x0112) lives in IFD0, FocalLengthIn35mmFilm (0xA405) in the Exif sub-IFD (0x8769).
ImageMetadata parse_exif(const std::vector<uint8_t>& e) {
    ImageMetadata m;
    if (e.size() < 8) return m;
    const bool le = e[0] == 'I' && e[1] == 'I';
    if (!le && !(e[0] == 'M' && e[1] == 'M')) return m;
    auto u16 = [&](size_t p) -> uint32_t { return p + 2 <= e.size() ? (le ? e[p] | (e[p + 1] << 8) : (e[p] << 8) | e[p + 1]) : 0u; };
    auto u32 = [&](size_t p) -> uint32_t {
        if (p + 4 > e.size()) return 0u;
        return le ? (uint32_t)e[p] | (e[p + 1] << 8) | (e[p + 2] << 16) | ((uint32_t)e[p + 3] << 24)
                  : ((uint32_t)e[p] << 24) | (e[p + 1] << 16) | (e[p + 2] << 8) | e[p + 3];
    };
    if (u16(2) != 42) return m;
    // value of an entry as an unsigned integer (BYTE, SHORT or LONG, first element)
    auto entry_uint = [&](size_t p, uint32_t* out) {
        const uint32_t type = u16(p + 2), count = u32(p + 4);
        if (count < 1) return false;
        if (type == 1) *out = e[p + 8];
        else if (type == 3) *out = u16(p + 8);
        else if (type == 4) *out = u32(p + 8);
        else return false;
        return true;
    };
    auto walk = [&](size_t ifd, auto&& on_entry) {
        if (ifd == 0 || ifd + 2 > e.size()) return;
        const uint32_t n = u16(ifd);
        for (uint32_t i = 0; i < n; ++i) {
            const size_t p = ifd + 2 + 12 * (size_t)i;
            if (p + 12 > e.size()) return;
            on_entry(u16(p), p);
        }
    };
    size_t exif_ifd = 0;
    walk(u32(4), [&](uint32_t tag, size_t p) {
        uint32_t v;
        if (tag == 0x0112 && entry_uint(p, &v) && v >= 1 && v <= 8) m.orientation = (int)v;
        if (tag == 0x8769 && entry_uint(p, &v)) exif_ifd = v;
        if (tag == 0xa405 && entry_uint(p, &v)) m.focal_length_35mm = v;
    });
    walk(exif_ifd, [&](uint32_t tag, size_t p) {
        uint32_t v;
        if (tag == 0xa405 && entry_uint(p, &v)) m.focal_length_35mm = v;
    });
    return m;
}

RgbImage apply_orientation(const RgbImage& img, int orientation) {
    if (orientation <= 1 || orientation > 8) return img;
    const uint32_t w = img.width, h = img.height;
    const bool swap = orientation >= 5;
    RgbImage out(swap ? h : w, swap ? w : h);
    for (uint32_t y = 0; y < out.height; ++y)
        for (uint32_t x = 0; x < out.width; ++x) {
            uint32_t sx, sy;  // source pixel of output (x, y)
            switch (orientation) {
                case 2: sx = w - 1 - x, sy = y; break;          // flip horizontally
                case 3: sx = w - 1 - x, sy = h - 1 - y; break;  // rotate 180
                case 4: sx = x, sy = h - 1 - y; break;          // flip vertically
                case 5: sx = y, sy = x; break;                  // transpose
                case 6: sx = y, sy = h - 1 - x; break;          // rotate 90 clockwise
                case 7: sx = w - 1 - y, sy = h - 1 - x; break;  // transverse
                default: sx = w - 1 - y, sy = x; break;         // 8: rotate 270 clockwise
            }
            std::memcpy(&out.data[((size_t)y * out.width + x) * 3], &img.data[((size_t)sy * w + sx) * 3], 3);
        }
    return out;
}

RgbImage load_image(const std::string& path, ImageMetadata* metadata) {
    const std::vector<uint8_t> file = read_file(path);
    std::vector<uint8_t> exif;
    RgbImage img;
    if (file.size() >= 8 && !std::memcmp(file.data(), kPngSig, 8))
        img = decode_png(file, path, &exif);
    else if (file.size() >= 3 && file[0] == 0xff && file[1] == 0xd8 && file[2] == 0xff)
        img = decode_jpeg(file, path, &exif);
    else if (file.size() >= 2 && file[0] == 'P' && file[1] == '6')
        img = decode_ppm(file, path);
    else
        throw ImageError(path + ": unsupported image format (this host layer decodes JPEG, PNG and binary PPM)");
    if (metadata) *metadata = parse_exif(exif);
    return img;
}

void save_image(const RgbImage& img, const std::string& path) {
    if (ends_with_ci(path, ".png")) return encode_png(img, path);
    if (ends_with_ci(path, ".ppm")) {
        std::ofstream f(path, std::ios::binary);
        f << "P6\n" << img.width << " " << img.height << "\n255\n";
        if (!f.write((const char*)img.data.data(), (std::streamsize)img.data.size())) throw ImageError("cannot write " + path);
        return;
    }
    if (ends_with_ci(path, ".jpg") || ends_with_ci(path, ".jpeg")) {
        const JpegOutputParams p = jpeg_output_params();
        const std::vector<uint8_t> file = encode_jpeg(img, p.quality, p.subsampling);
        std::ofstream f(path, std::ios::binary);
        if (!f.write((const char*)file.data(), (std::streamsize)file.size())) throw ImageError("cannot write " + path);
        return;
    }
    throw ImageError(path + ": unsupported output image format (this host layer encodes .png, .jpg / .jpeg and .ppm)");
}

RgbImage resize_exact_lanczos3(const RgbImage& img, uint32_t width, uint32_t height) {
    if (img.width == width && img.height == height) return img;
    if (!width || !height || !img.width || !img.height) throw ImageError("resize to or from an empty image");
    std::vector<float> src(img.data.begin(), img.data.end());
    // vertical pass first, then horizontal (the order the image crate uses)
    std::vector<float> mid((size_t)img.width * height * 3);
    resample(src, mid, img.height, height, img.width, (size_t)img.width * 3, 3, (size_t)img.width * 3, 3);
    std::vector<float> dst((size_t)width * height * 3);
    resample(mid, dst, img.width, width, height, 3, (size_t)img.width * 3, 3, (size_t)width * 3);
    RgbImage out(width, height);
    for (size_t i = 0; i < dst.size(); ++i) out.data[i] = (uint8_t)std::lround(std::min(255.0f, std::max(0.0f, dst[i])));
    return out;
}

}  // namespace matrix_eyes
