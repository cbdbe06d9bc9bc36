// Baseline JPEG encoding (RgbImage::save to ".jpg", output.rs:138 and :192), byte for byte the file libjpeg writes with its
// default integer path and the Annex K tables (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jchuff.c; optimize off):
//
//   fdct     8 lanes per block, blocks in SCAN order (MCU by MCU, luma blocks row by row, then Cb, then Cr), dummy blocks of
//            partial MCUs included.  A lane gathers one row of the block's samples straight from the RGB picture -- colour
//            conversion, libjpeg's edge replication and its h2v1 / h2v2 down-sampling applied per sample, no plane is ever
//            stored -- and runs the row pass; after the transpose a lane owns a column, runs the column pass, quantises and
//            stores int16 coefficients in zigzag order.  A dummy block is the nearest real block before it in its MCU with
//            every AC coefficient dropped, so no block depends on another one.
//   bits     one lane per zigzag position: from the mask of the block's non-zero positions a lane knows the zero run in front
//            of it, hence its ZRLs, its symbol and its magnitude bits (at most 3 * 11 + 16 + 10 = 59 bits).  Lane 0 codes the
//            DC difference against the previous block of its component in scan order, lane 63 the EOB of a block that ends in
//            zeros.  A block's length is the sum over its lanes.
//   pack     the same codes again, ORed into a zeroed big-endian word stream at the exclusive sum of all lengths before them
//   stuff    per 16 bytes of that stream: count the FF bytes; after a second exclusive sum, scatter with 00 behind each FF
//
// The per-lane routines are plain functions: the bodies of the kernels of csrc/jpeg_encode.hip and, with ME_JPEG_HOST
// defined, plain C++ that tests/jpeg_encode_host.cpp runs lane by lane.  The host half (tables and the file header) is the
// same code in both builds and in host/jpeg_encoder.cpp.
#pragma once
#ifndef ME_JPEG_HOST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include <initializer_list>

namespace me_jpeg_encode {

#ifdef ME_JPEG_HOST
#define JC_FN inline
#else
#define JC_FN __device__ inline
#endif

constexpr int kThreads = 256;
constexpr int kFdctBlocks = kThreads / 8;    // blocks per workgroup of the fdct kernel
constexpr int kWaveBlocks = kThreads / 64;   // ... of the bits and pack kernels
constexpr int kTileStride = 9;               // dwords per row of a block in LDS (8 + 1 against bank conflicts)
constexpr int kStuffBytes = 16;              // bytes of the packed stream per lane of the stuffing kernels
constexpr int kMaxLaneBits = 59;
constexpr int kMaxHeader = 640;              // the header is 623 bytes
constexpr int kMaxDim = 65535;               // SOF0 holds 16 bits per side

// zigzag position -> natural index, and back
constexpr uint8_t kZigzagNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kNaturalZigzag[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                        41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                        46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct EncDesc {
    int32_t w, h, hs, vs;            // picture; luma sampling factors (chroma is 1 x 1)
    int32_t mcus_x, mcus_y, nb;      // MCUs; blocks per MCU (hs * vs + 2)
    int32_t wb, hb;                  // real luma blocks per row and column
    int32_t total_blocks;            // of the scan, dummies included
    int32_t header_len, reserved;
};
struct EncCodes {
    uint16_t q[2][64];               // quantisation tables, natural order
    uint32_t dc[2][16];              // category -> length << 16 | code
    uint32_t ac[2][256];             // symbol -> length << 16 | code
    EncDesc d;
};
struct EncTables {
    EncCodes c;
    uint8_t header[kMaxHeader];      // SOI .. SOS
};
static_assert(sizeof(EncCodes) % 4 == 0 && sizeof(EncTables) % 4 == 0, "staged as dwords");

JC_FN int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }

// ---- scan order ---------------------------------------------------------------------------------------------------------
struct BlockAt {
    int32_t comp, bx, by;            // the block whose samples make block i: itself, or for a dummy the real block before it
    bool dummy;
};
JC_FN BlockAt block_at(const EncDesc& d, int32_t i) {
    const int32_t m = i / d.nb, my = m / d.mcus_x, mx = m - my * d.mcus_x, ny = d.hs * d.vs;
    int32_t b = i - m * d.nb;
    BlockAt a;
    a.dummy = false;
    if (b >= ny) {
        a.comp = 1 + (b - ny), a.bx = mx, a.by = my;
        return a;
    }
    a.comp = 0;
    for (;; --b) {  // block 0 of an MCU is real: at most three steps back
        a.bx = mx * d.hs + b % d.hs, a.by = my * d.vs + b / d.hs;
        if (a.bx < d.wb && a.by < d.hb) break;
        a.dummy = true;
    }
    return a;
}
// the block whose DC predicts block i's: the one before it of the same component in scan order; -1: none (predictor 0)
JC_FN int32_t dc_predecessor(const EncDesc& d, int32_t i) {
    const int32_t m = i / d.nb, b = i - m * d.nb, ny = d.hs * d.vs;
    if (b < ny) return b > 0 ? i - 1 : (m > 0 ? (m - 1) * d.nb + ny - 1 : -1);
    return m > 0 ? i - d.nb : -1;
}

// ---- samples ------------------------------------------------------------------------------------------------------------
constexpr int32_t fix16(double x) { return (int32_t)(x * 65536.0 + 0.5); }
// jccolor.c rgb_ycc_convert
JC_FN int32_t convert(const uint8_t* p, int comp) {
    const int32_t r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (fix16(0.299) * r + fix16(0.587) * g + fix16(0.114) * b + 32768) >> 16;
    if (comp == 1) return (-fix16(0.16874) * r - fix16(0.33126) * g + fix16(0.5) * b + (128 << 16) + 32767) >> 16;
    return (fix16(0.5) * r - fix16(0.41869) * g - fix16(0.08131) * b + (128 << 16) + 32767) >> 16;
}
// Sample (x, y) of a component's padded plane.  Luma and full-resolution chroma replicate the picture's last column and row.
// Down-sampled chroma in libjpeg's order: the full-resolution plane is replicated to the right as far as needed and downward
// only to a multiple of vs rows, then averaged (bias 1, 2, 1, 2 ... for h2v2 and 0, 1, 0, 1 ... for h2v1), and it is the
// DOWN-SAMPLED last row that is replicated further down.
JC_FN int32_t sample(const EncDesc& d, const uint8_t* rgb, int comp, int32_t x, int32_t y) {
    const int64_t stride = (int64_t)d.w * 3;
    if (comp == 0 || d.hs == 1) return convert(rgb + imin(y, d.h - 1) * stride + (int64_t)imin(x, d.w - 1) * 3, comp);
    const int64_t x0 = (int64_t)imin(2 * x, d.w - 1) * 3, x1 = (int64_t)imin(2 * x + 1, d.w - 1) * 3;
    if (d.vs == 1) {
        const uint8_t* row = rgb + imin(y, d.h - 1) * stride;
        return (convert(row + x0, comp) + convert(row + x1, comp) + (x & 1)) >> 1;
    }
    const int32_t oy = imin(y, (d.h + 1) / 2 - 1);
    const uint8_t* r0 = rgb + imin(2 * oy, d.h - 1) * stride;
    const uint8_t* r1 = rgb + imin(2 * oy + 1, d.h - 1) * stride;
    return (convert(r0 + x0, comp) + convert(r0 + x1, comp) + convert(r1 + x0, comp) + convert(r1 + x1, comp) + 1 + (x & 1)) >> 2;
}

// ---- FDCT and quantisation ----------------------------------------------------------------------------------------------
JC_FN int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }
// jfdctint.c (CONST_BITS 13, PASS1_BITS 2), one row (first) or one column of a block
JC_FN void fdct_pass(int32_t v[8], bool first) {
    const int32_t t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
    const int32_t t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = first ? 13 - 2 : 13 + 2;
    v[0] = first ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    v[4] = first ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int32_t z1 = (t12 + t13) * 4433;
    v[2] = descale(z1 + t13 * 6270, n);
    v[6] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    v[7] = descale(u4 + z1 + z3, n);
    v[5] = descale(u5 + z2 + z4, n);
    v[3] = descale(u6 + z2 + z3, n);
    v[1] = descale(u7 + z1 + z4, n);
}
// jcdctmgr.c: the coefficient carries a factor 8
JC_FN int32_t quantise(int32_t v, int32_t q) {
    const int32_t qv = q << 3;
    const int32_t a = ((v < 0 ? -v : v) + (qv >> 1)) / qv;
    return v < 0 ? -a : a;
}

// lane r of block i, first half: row r of the block after the row pass -> tile_row[0..7]
JC_FN void fdct_row_lane(const EncDesc& d, const uint8_t* rgb, int32_t i, int r, int32_t* tile_row) {
    const BlockAt a = block_at(d, i);
    int32_t v[8];
    for (int c = 0; c < 8; ++c) v[c] = sample(d, rgb, a.comp, a.bx * 8 + c, a.by * 8 + r) - 128;
    fdct_pass(v, true);
    for (int c = 0; c < 8; ++c) tile_row[c] = v[c];
}
// lane c of block i, second half: column c of `tile` (rows `stride` dwords apart) -> eight coefficients of coef[i * 64 ...]
JC_FN void fdct_col_lane(const EncCodes& T, int32_t i, int c, const int32_t* tile, int stride, int16_t* coef) {
    const BlockAt a = block_at(T.d, i);
    const uint16_t* q = T.q[a.comp ? 1 : 0];
    int32_t v[8];
    for (int r = 0; r < 8; ++r) v[r] = tile[r * stride + c];
    fdct_pass(v, false);
    for (int r = 0; r < 8; ++r) {
        const int n = r * 8 + c;
        const int32_t qv = a.dummy && n != 0 ? 0 : quantise(v[r], q[n]);
        coef[(int64_t)i * 64 + kNaturalZigzag[n]] = (int16_t)qv;
    }
}

// ---- Huffman codes ------------------------------------------------------------------------------------------------------
struct LaneCode {
    uint64_t bits;                   // right-aligned
    int32_t len;                     // 0 .. kMaxLaneBits
};
JC_FN int bit_length(uint32_t a) { return a ? 32 - __builtin_clz(a) : 0; }
JC_FN uint32_t magnitude_bits(int32_t v, int n) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// What lane k (zigzag position k) of block i writes: v its coefficient, nz the mask of the block's non-zero positions
JC_FN LaneCode lane_code(const EncCodes& T, const int16_t* coef, int32_t i, int k, int32_t v, uint64_t nz) {
    const EncDesc& d = T.d;
    const int t = i % d.nb >= d.hs * d.vs ? 1 : 0;
    LaneCode c;
    c.bits = 0, c.len = 0;
    if (k == 0) {
        const int32_t p = dc_predecessor(d, i);
        const int32_t diff = v - (p < 0 ? 0 : (int32_t)coef[(int64_t)p * 64]);
        const int n = bit_length((uint32_t)(diff < 0 ? -diff : diff));
        const uint32_t e = T.dc[t][n];
        c.len = (int32_t)(e >> 16) + n;
        c.bits = ((uint64_t)(e & 0xffffu) << n) | magnitude_bits(diff, n);
        return c;
    }
    if (v == 0) {
        if (k == 63) {  // the block ends in zeros: EOB
            const uint32_t e = T.ac[t][0];
            c.len = (int32_t)(e >> 16), c.bits = e & 0xffffu;
        }
        return c;
    }
    const uint64_t before = nz & ((1ull << k) - 1ull) & ~1ull;     // non-zero AC positions in front of k
    int run = k - 1 - (before ? 63 - __builtin_clzll(before) : 0);
    const uint32_t zrl = T.ac[t][0xf0];
    for (; run > 15; run -= 16) {  // at most three
        c.bits = (c.bits << (zrl >> 16)) | (zrl & 0xffffu);
        c.len += (int32_t)(zrl >> 16);
    }
    const int n = bit_length((uint32_t)(v < 0 ? -v : v));
    const uint32_t e = T.ac[t][(run << 4) | n];
    const int l = (int)(e >> 16) + n;
    c.bits = (c.bits << l) | ((uint64_t)(e & 0xffffu) << n) | magnitude_bits(v, n);
    c.len += l;
    return c;
}

JC_FN void or_word(uint32_t* word, uint32_t v) {
#ifdef ME_JPEG_HOST
    *word |= v;
#else
    atomicOr(word, v);  // OR commutes: the stream does not depend on the order
#endif
}
// ORs the low `len` (<= kMaxLaneBits) bits of `bits` into the big-endian bit stream `words` at bit `at`; only words that
// receive a set bit are touched
JC_FN void put_bits(uint32_t* words, uint64_t at, uint64_t bits, int len) {
    if (len <= 0) return;
    const uint64_t w = at >> 5;
    const int sh = (int)(at & 31);
    const uint64_t left = bits << (64 - len);
    const uint64_t head = left >> sh;
    const uint32_t w0 = (uint32_t)(head >> 32), w1 = (uint32_t)head;
    const uint32_t w2 = sh ? (uint32_t)((left << (64 - sh)) >> 32) : 0u;
    if (w0) or_word(words + w, __builtin_bswap32(w0));
    if (w1) or_word(words + w + 1, __builtin_bswap32(w1));
    if (w2) or_word(words + w + 2, __builtin_bswap32(w2));
}

// ---- byte stuffing ------------------------------------------------------------------------------------------------------
// `words` is the packed stream, zero-filled to a multiple of kStuffBytes: a lane owns kStuffBytes of it
JC_FN uint32_t count_ff(const uint32_t* words, int64_t chunk) {
    uint32_t n = 0;
    for (int j = 0; j < kStuffBytes / 4; ++j) {
        const uint32_t w = words[chunk * (kStuffBytes / 4) + j];
        for (int b = 0; b < 4; ++b) n += ((w >> (8 * b)) & 255u) == 255u ? 1u : 0u;
    }
    return n;
}
// the lane's bytes (those in front of `nbytes`) to out[chunk * kStuffBytes + ff_before ...], 00 behind each FF
JC_FN void stuff_chunk(const uint32_t* words, int64_t nbytes, int64_t chunk, uint64_t ff_before, uint8_t* out) {
    int64_t at = chunk * kStuffBytes;
    uint8_t* o = out + at + (int64_t)ff_before;
    for (int j = 0; j < kStuffBytes / 4; ++j) {
        const uint32_t w = words[chunk * (kStuffBytes / 4) + j];
        for (int b = 0; b < 4 && at < nbytes; ++b, ++at) {
            const uint8_t v = (uint8_t)(w >> (8 * b));
            *o++ = v;
            if (v == 255u) *o++ = 0;
        }
    }
}

// ---- the host half: tables and header -----------------------------------------------------------------------------------
constexpr uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// T.81 Annex K.3
constexpr uint8_t kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcValues[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// canonical codes of one table: symbol values[k] -> length << 16 | code
inline void build_codes(const uint8_t counts[16], const uint8_t* values, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int j = 0; j < counts[len - 1]; ++j) out[values[k++]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
}

inline bool valid_parameters(int64_t w, int64_t h, int quality, int subsampling) {
    return w > 0 && h > 0 && w <= kMaxDim && h <= kMaxDim && quality >= 1 && quality <= 100 && subsampling >= 0 && subsampling <= 2;
}

// quantisation tables, codes, geometry and the file's header (SOI, APP0, 2 DQT, SOF0, 4 DHT, SOS) for one picture;
// subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
inline void build_tables(int32_t w, int32_t h, int quality, int subsampling, EncTables& t) {
    memset(&t, 0, sizeof(t));
    EncDesc& d = t.c.d;
    d.w = w, d.h = h, d.hs = subsampling == 0 ? 1 : 2, d.vs = subsampling == 2 ? 2 : 1;
    d.mcus_x = (w + 8 * d.hs - 1) / (8 * d.hs), d.mcus_y = (h + 8 * d.vs - 1) / (8 * d.vs), d.nb = d.hs * d.vs + 2;
    d.wb = (w + 7) / 8, d.hb = (h + 7) / 8;
    d.total_blocks = d.mcus_x * d.mcus_y * d.nb;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < 64; ++i) {
            const int v = (kBaseQ[s][i] * scale + 50) / 100;
            t.c.q[s][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    uint8_t dc_values[12];
    for (int i = 0; i < 12; ++i) dc_values[i] = (uint8_t)i;
    for (int s = 0; s < 2; ++s) {
        build_codes(kDcCounts[s], dc_values, t.c.dc[s]);
        build_codes(kAcCounts[s], kAcValues[s], t.c.ac[s]);
    }
    uint8_t* p = t.header;
    auto put = [&](std::initializer_list<int> bytes) {
        for (int b : bytes) *p++ = (uint8_t)b;
    };
    put({0xff, 0xd8, 0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int s = 0; s < 2; ++s) {
        put({0xff, 0xdb, 0x00, 0x43, s});
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)t.c.q[s][kZigzagNatural[k]];
    }
    put({0xff, 0xc0, 0x00, 0x11, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, d.hs << 4 | d.vs, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int s = 0; s < 2; ++s) {
        put({0xff, 0xc4, 0x00, 19 + 12, s});
        memcpy(p, kDcCounts[s], 16), p += 16;
        memcpy(p, dc_values, 12), p += 12;
        put({0xff, 0xc4, 0x00, 19 + 162, 0x10 | s});
        memcpy(p, kAcCounts[s], 16), p += 16;
        memcpy(p, kAcValues[s], 162), p += 162;
    }
    put({0xff, 0xda, 0x00, 0x0c, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3f, 0});
    d.header_len = (int32_t)(p - t.header);
}

}  // namespace me_jpeg_encode
