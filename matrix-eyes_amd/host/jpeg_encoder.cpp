// RgbImage::save to ".jpg" / ".jpeg" (output.rs:138, :192) for the C++ host layer: a sequential baseline encoder that writes,
// byte for byte, the file libjpeg writes with its integer path and the Annex K tables (csrc/jpeg_encode.h says which rules
// those are and holds the arithmetic of a sample, a row and a coefficient).  Unlike the device path it is the textbook
// form: whole colour planes, padded and down-sampled in libjpeg's order, block after block through one bit writer that
// stuffs as it goes.
#define ME_JPEG_HOST
#include "../csrc/jpeg_encode.h"

#include <algorithm>
#include <cstdlib>
#include <fstream>

#include "image_io.hpp"

namespace matrix_eyes {

namespace {

using namespace me_jpeg_encode;

struct Plane {
    int w = 0, h = 0;
    std::vector<int32_t> v;
    Plane(int w_, int h_) : w(w_), h(h_), v((size_t)w_ * h_) {}
    int32_t& at(int x, int y) { return v[(size_t)y * w + x]; }
    int32_t at(int x, int y) const { return v[(size_t)y * w + x]; }
};

// edge replication to `w` columns and `h` rows
Plane expanded(const Plane& p, int w, int h) {
    Plane out(w, h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) out.at(x, y) = p.at(std::min(x, p.w - 1), std::min(y, p.h - 1));
    return out;
}

struct BitWriter {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t code, int len) {
        acc = (acc << len) | (code & ((1u << len) - 1u));
        n += len;
        while (n >= 8) {
            n -= 8;
            const uint8_t b = (uint8_t)(acc >> n);
            out.push_back(b);
            if (b == 0xff) out.push_back(0);
        }
    }
    void put_entry(uint32_t e) { put(e & 0xffffu, (int)(e >> 16)); }
    void finish() {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

int parse_int(const char* name, const char* text, int lo, int hi) {
    char* end = nullptr;
    const long v = std::strtol(text, &end, 10);
    if (end == text || *end || v < lo || v > hi)
        throw ImageError(std::string(name) + "=" + text + ": expected an integer in " + std::to_string(lo) + ".." + std::to_string(hi));
    return (int)v;
}

}  // namespace

std::vector<uint8_t> encode_jpeg(const RgbImage& img, int quality, int subsampling) {
    if (!valid_parameters(img.width, img.height, quality, subsampling) || img.data.size() != (size_t)img.width * img.height * 3)
        throw ImageError("encode_jpeg: " + std::to_string(img.width) + "x" + std::to_string(img.height) + ", quality " +
                         std::to_string(quality) + ", subsampling " + std::to_string(subsampling) +
                         ": sides of 1..65535, quality 1..100, subsampling 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
    const int w = (int)img.width, h = (int)img.height;
    std::vector<EncTables> tables(1);
    build_tables(w, h, quality, subsampling, tables[0]);
    const EncCodes& T = tables[0].c;
    const int hs = T.d.hs, vs = T.d.vs;

    // the three planes in blocks: luma at full resolution, chroma down-sampled
    std::vector<Plane> planes;
    for (int c = 0; c < 3; ++c) {
        Plane full(w, h);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) full.at(x, y) = convert(&img.data[((size_t)y * w + x) * 3], c);
        const int fx = c ? hs : 1, fy = c ? vs : 1;
        const int wb = ((w + fx - 1) / fx + 7) / 8, hb = ((h + fy - 1) / fy + 7) / 8;
        if (fx == 1) {
            planes.push_back(expanded(full, wb * 8, hb * 8));
            continue;
        }
        const Plane wide = expanded(full, wb * 16, (h + fy - 1) / fy * fy);
        Plane down(wb * 8, wide.h / fy);
        for (int y = 0; y < down.h; ++y)
            for (int x = 0; x < down.w; ++x)
                down.at(x, y) = fy == 2 ? (wide.at(2 * x, 2 * y) + wide.at(2 * x + 1, 2 * y) + wide.at(2 * x, 2 * y + 1) +
                                           wide.at(2 * x + 1, 2 * y + 1) + 1 + (x & 1)) >> 2
                                        : (wide.at(2 * x, y) + wide.at(2 * x + 1, y) + (x & 1)) >> 1;
        planes.push_back(expanded(down, wb * 8, hb * 8));
    }
    // one block's quantised coefficients in zigzag order
    auto transform = [&](int c, int bx, int by, int32_t* zz) {
        const Plane& p = planes[(size_t)c];
        int32_t blk[8][8], col[8];
        for (int y = 0; y < 8; ++y) {
            for (int x = 0; x < 8; ++x) blk[y][x] = p.at(bx * 8 + x, by * 8 + y) - 128;
            fdct_pass(blk[y], true);
        }
        for (int x = 0; x < 8; ++x) {
            for (int y = 0; y < 8; ++y) col[y] = blk[y][x];
            fdct_pass(col, false);
            for (int y = 0; y < 8; ++y) zz[kNaturalZigzag[y * 8 + x]] = quantise(col[y], T.q[c ? 1 : 0][y * 8 + x]);
        }
    };

    std::vector<uint8_t> out(tables[0].header, tables[0].header + T.d.header_len);
    out.reserve(out.size() + (size_t)w * h / 2 + 1024);
    BitWriter bits{out};
    int32_t pred[3] = {0, 0, 0};
    for (int my = 0; my < T.d.mcus_y; ++my)
        for (int mx = 0; mx < T.d.mcus_x; ++mx) {
            int32_t zz[64] = {0};
            for (int b = 0; b < T.d.nb; ++b) {
                const int c = b < hs * vs ? 0 : 1 + (b - hs * vs);
                const int bx = c ? mx : mx * hs + b % hs, by = c ? my : my * vs + b / hs;
                if (c == 0 && (bx >= T.d.wb || by >= T.d.hb)) {
                    for (int k = 1; k < 64; ++k) zz[k] = 0;  // a dummy block: the DC of the block before it, nothing else
                } else {
                    transform(c, bx, by, zz);
                }
                const int t = c ? 1 : 0;
                const int32_t diff = zz[0] - pred[c];
                pred[c] = zz[0];
                int n = bit_length((uint32_t)std::abs(diff));
                bits.put_entry(T.dc[t][n]);
                if (n) bits.put(magnitude_bits(diff, n), n);
                int run = 0;
                for (int k = 1; k < 64; ++k) {
                    if (zz[k] == 0) {
                        ++run;
                        continue;
                    }
                    for (; run > 15; run -= 16) bits.put_entry(T.ac[t][0xf0]);
                    n = bit_length((uint32_t)std::abs(zz[k]));
                    bits.put_entry(T.ac[t][(run << 4) | n]);
                    bits.put(magnitude_bits(zz[k], n), n);
                    run = 0;
                }
                if (run) bits.put_entry(T.ac[t][0]);
            }
        }
    bits.finish();
    out.push_back(0xff), out.push_back(0xd9);
    return out;
}

JpegOutputParams jpeg_output_params() {
    JpegOutputParams p;
    if (const char* q = std::getenv("MATRIX_EYES_JPEG_QUALITY")) p.quality = parse_int("MATRIX_EYES_JPEG_QUALITY", q, 1, 100);
    if (const char* s = std::getenv("MATRIX_EYES_JPEG_SUBSAMPLING")) {
        const std::string v = s;
        if (v == "4:4:4") p.subsampling = 0;
        else if (v == "4:2:2") p.subsampling = 1;
        else if (v == "4:2:0") p.subsampling = 2;
        else throw ImageError("MATRIX_EYES_JPEG_SUBSAMPLING=" + v + ": expected 4:4:4, 4:2:2 or 4:2:0");
    }
    return p;
}

}  // namespace matrix_eyes
