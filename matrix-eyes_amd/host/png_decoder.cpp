// The PNG decoder of the C++ host layer (the reference's `image` crate with the "png" feature: reconstruction.rs:95-113,
// output.rs:206-218), cut at the seam the device decoder (csrc/png_decode.hip) needs: parse_png_header reads the chunks,
// inflate_png turns the IDAT data into the filtered stream, and decode_png is those two plus the reconstruction.  The
// reconstruction's arithmetic is csrc/png_recon.h's, shared with the kernels.
#include <zlib.h>

#include <algorithm>
#include <cstring>

#include "../csrc/png_recon.h"
#include "image_io.hpp"

namespace matrix_eyes {

namespace {

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

const char* const kNoInflate = ": PNG data does not inflate to the image size";

}  // namespace

PngFrame parse_png_header(const std::vector<uint8_t>& file, const std::string& path) {
    PngFrame f;
    size_t pos = 8;
    uint32_t width = 0, height = 0;
    int depth = 0, ctype = -1, interlace = 0;
    while (pos + 12 <= file.size()) {
        const uint32_t len = be32(&file[pos]);
        const char* type = (const char*)&file[pos + 4];
        if (pos + 12 + len > file.size()) throw ImageError(path + ": truncated PNG chunk");
        const uint8_t* body = &file[pos + 8];
        if (!std::memcmp(type, "IHDR", 4)) {
            if (len < 13) throw ImageError(path + ": bad IHDR");
            width = be32(body), height = be32(body + 4);
            depth = body[8], ctype = body[9], interlace = body[12];
        } else if (!std::memcmp(type, "PLTE", 4)) {
            f.plte.assign(body, body + len);
        } else if (!std::memcmp(type, "eXIf", 4)) {
            f.exif_offset = pos + 8, f.exif_nbytes = len;   // the last one counts
        } else if (!std::memcmp(type, "IDAT", 4)) {
            f.idat.push_back({pos + 8, (size_t)len});
        } else if (!std::memcmp(type, "IEND", 4)) {
            break;
        }
        pos += 12 + (size_t)len;
    }
    if (!width || !height || ctype < 0) throw ImageError(path + ": no IHDR");
    if ((int64_t)width * height > kMaxPixels) throw ImageError(path + ": PNG larger than 2^28 pixels");
    if (interlace > 1) throw ImageError(path + ": bad PNG interlace method");
    if (depth != 1 && depth != 2 && depth != 4 && depth != 8 && depth != 16)
        throw ImageError(path + ": bad PNG bit depth " + std::to_string(depth));
    const int channels = me_pngdec::channels_of(ctype);
    if (!channels) throw ImageError(path + ": bad PNG colour type");
    // PNG spec table 11.1: sub-byte depths for grey and palette only, 16 bit not for palette
    if ((depth < 8 && ctype != 0 && ctype != 3) || (depth == 16 && ctype == 3))
        throw ImageError(path + ": PNG bit depth " + std::to_string(depth) + " does not go with colour type " +
                         std::to_string(ctype));
    f.width = width, f.height = height, f.depth = depth, f.ctype = ctype, f.interlace = interlace;
    f.geom = me_pngdec::make_geom((int32_t)width, (int32_t)height, depth, ctype, interlace);
    f.bits_pp = f.geom.bits_pp, f.bpp = f.geom.bpp, f.total = (size_t)f.geom.total;
    return f;
}

void inflate_png(const PngFrame& frame, const std::vector<uint8_t>& file, const std::string& path, uint8_t* dst,
                 PngBandCallback band_cb, void* band_user) {
    constexpr size_t kStep = 256 * 1024;   // stream bytes between two calls of band_cb
    z_stream z;
    std::memset(&z, 0, sizeof(z));
    if (inflateInit(&z) != Z_OK) throw ImageError(path + kNoInflate);
    struct Guard {
        z_stream* z;
        ~Guard() { inflateEnd(z); }
    } guard{&z};
    const size_t total = frame.total;
    size_t done = 0, span = 0;
    uint8_t spill;          // where a byte past `total` would go: the stream then runs long
    bool ended = false;
    while (!ended) {
        if (z.avail_in == 0) {
            while (span < frame.idat.size() && frame.idat[span].nbytes == 0) ++span;
            if (span == frame.idat.size()) break;   // the data ends before the stream does
            z.next_in = const_cast<Bytef*>(&file[frame.idat[span].offset]);
            z.avail_in = (uInt)frame.idat[span].nbytes;
            ++span;
        }
        const size_t room = std::min(kStep, total - done);
        z.next_out = room ? dst + done : &spill;
        z.avail_out = room ? (uInt)room : 1u;
        const int rc = inflate(&z, Z_NO_FLUSH);
        const size_t made = (room ? room : 1u) - z.avail_out;
        if (!room && made) throw ImageError(path + kNoInflate);   // more than the picture holds
        done += made;
        if (rc == Z_STREAM_END) ended = true;   // the Adler-32 has been checked; what follows inside IDAT is ignored
        else if (rc != Z_OK && !(rc == Z_BUF_ERROR && z.avail_in == 0)) throw ImageError(path + kNoInflate);
        if (band_cb && made) band_cb(band_user, done);
    }
    if (!ended || done != total) throw ImageError(path + kNoInflate);
}

RgbImage decode_png(const std::vector<uint8_t>& file, const std::string& path, std::vector<uint8_t>* exif) {
    const PngFrame f = parse_png_header(file, path);
    if (exif && f.exif_nbytes) exif->assign(file.begin() + (ptrdiff_t)f.exif_offset, file.begin() + (ptrdiff_t)(f.exif_offset + f.exif_nbytes));
    std::vector<uint8_t> raw(f.total);
    inflate_png(f, file, path, raw.data());
    RgbImage img(f.width, f.height);
    const me_pngdec::Geom& g = f.geom;
    for (int ps = 0; ps < g.npass; ++ps) {
        const me_pngdec::Pass& p = g.pass[ps];
        if (!p.pw || !p.ph) continue;
        const size_t stride = (size_t)p.stride, bpp = (size_t)g.bpp;
        std::vector<uint8_t> prev(stride, 0);
        for (int32_t py = 0; py < p.ph; ++py) {
            uint8_t* row = &raw[(size_t)p.offset + (size_t)py * (stride + 1) + 1];
            const int filter = row[-1];
            if (filter > 4) throw ImageError(path + ": bad PNG filter");
            // undo the scanline filter in place
            for (size_t i = 0; i < stride; ++i) {
                const int a = i >= bpp ? row[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
                row[i] = me_pngdec::recon(filter, row[i], a, b, c);
            }
            std::memcpy(prev.data(), row, stride);
            for (int32_t px = 0; px < p.pw; ++px) {
                uint8_t* out = &img.data[(size_t)me_pngdec::dest_index(g, p, px, py, 1) * 3];
                if (!me_pngdec::pixel_rgb(g, row, px, f.plte.data(), (int32_t)f.plte.size(), out))
                    throw ImageError(path + ": palette index out of range");
            }
        }
    }
    return img;
}

}  // namespace matrix_eyes
