// Reconstruction of a JPEG picture from its quantised DCT coefficients, as host/jpeg_decoder.cpp does it (Decoder::idct_all,
// upsample, finish) and byte for byte: dequantisation, the DC-only shortcut, the separable IDCT in double precision, level
// shift, libjpeg's "fancy" chroma upsampling, the 16-bit fixed-point JFIF colour conversion and the EXIF orientation.
//
// The per-block routine is written as a sequence of PHASES -- JPEG_LANES { code of lane t of 64 } JPEG_SYNC -- with every
// value that lives across a phase in the block's shared struct, so that the same text is the body of a HIP kernel (a block =
// one wave, a phase = the code of lane t, JPEG_SYNC = __syncthreads) and, with ME_JPEG_HOST defined, plain C++ that runs a
// phase lane by lane (tests/jpeg_recon_host.cpp: the arithmetic is checked against the host decoder without a GPU).  The
// per-pixel routines are pure functions of the planes.
//
// Rounding: every f64 multiply and add is rounded once (the host decoder is g++ -O2 on x86-64, which has no FMA to contract
// into); the unit that includes this header is compiled with -ffp-contract=off and the products go through jpeg_mul /
// jpeg_add, which are the never-fused intrinsics on the device.
#pragma once
#ifndef ME_JPEG_HOST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include "orient.h"

namespace me_jpeg {

constexpr int kLanes = 64;          // lanes of one 8x8 block: lane t makes sample t
constexpr int kRow = 9;             // doubles per staged row of 8: rows 72 bytes apart start in different LDS banks
constexpr int kMaxComps = 3;

enum UpMode : int32_t {
    UP_COPY = 0,   // 1x1
    UP_H2V1 = 1,   // libjpeg h2v1_fancy_upsample (components wider than 2 samples)
    UP_H2V2 = 2,   // libjpeg h2v2_fancy_upsample (the same)
    UP_H1V2 = 3,   // libjpeg-turbo h1v2_fancy_upsample
    UP_REPL = 4    // every other integer ratio, and 2x1 / 2x2 of a component at most 2 samples wide: replication
};
enum ColorMode : int32_t { COLOR_GREY = 0, COLOR_RGB = 1, COLOR_YCC = 2 };

struct CompDesc {
    int32_t width, height;       // samples of the component
    int32_t blocks_w, blocks_h;  // allocated blocks (whole MCUs)
    int32_t pw;                  // bytes per plane row: blocks_w * 8
    int32_t fx, fy, mode;        // hmax / h, vmax / v, UpMode
    int32_t block0;              // index of the component's first block among all blocks of the frame
    int32_t qsel;                // which of the frame's tables (0..2: the component's own copy)
    int64_t coef_off;            // int16_t index of its first coefficient
    int64_t plane_off;           // byte offset of its plane (a multiple of 8)
};
struct Frame {
    int32_t width, height;       // of the decoded picture, before the orientation
    int32_t ncomp, color;        // 1 or 3; ColorMode
    int32_t orientation;         // 1..8
    int32_t total_blocks;
    CompDesc comp[kMaxComps];
};
struct IdctTables {
    double basis[64];            // basis[x * 8 + u] (csrc/jpeg_basis.cpp)
    uint16_t q[kMaxComps][64];   // per component, natural order
};

// what lives across the phases of one block
struct BlockShared {
    double in[8 * kRow];         // dequantised coefficients, row v at v * kRow
    double tmp[8 * kRow];        // after the row pass
    uint8_t px[64];
    int32_t any_ac;              // some AC COEFFICIENT (not product) of the block is not zero
};

#ifdef ME_JPEG_HOST
#define JPEG_FN inline
#define JPEG_LANES for (int t = 0; t < ::me_jpeg::kLanes; ++t) { if (active) {
#define JPEG_SYNC } }
#define JPEG_VOTE_ANY(flag, pred) do { if (pred) (flag) = 1; } while (0)
inline double jpeg_mul(double a, double b) { return a * b; }
inline double jpeg_add(double a, double b) { return a + b; }
inline double jpeg_trunc(double a) { return __builtin_trunc(a); }
#else
#define JPEG_FN __device__ inline
#define JPEG_LANES { const int t = (int)(threadIdx.x & 63u); if (active) {
#define JPEG_SYNC } } __syncthreads();
// one block = one wave: the vote is the wave's
#define JPEG_VOTE_ANY(flag, pred) do { const int any__ = __any((pred) ? 1 : 0); if (t == 0) (flag) = any__; } while (0)
__device__ inline double jpeg_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ inline double jpeg_add(double a, double b) { return __dadd_rn(a, b); }
__device__ inline double jpeg_trunc(double a) { return trunc(a); }
#endif

// (int)std::lround(s): half away from zero; s - trunc(s) is exact.  Beyond the int range the host's conversion of the long keeps
// the low 32 bits, as this one does.
JPEG_FN int32_t round_to_int(double s) {
    double r = jpeg_trunc(s);
    const double frac = s - r;
    if (frac >= 0.5) r += 1.0;
    if (frac <= -0.5) r -= 1.0;
    return (int32_t)(uint32_t)(uint64_t)(int64_t)r;
}
JPEG_FN uint8_t clamp_u8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// One 8x8 block: coef (64, natural order) and q (the component's table) -> out (8 rows, pw bytes apart, 8-byte aligned).
// `active`: uniform over the block's lanes; an inactive block only keeps the barriers company.
JPEG_FN void idct_block(BlockShared& sh, bool active, const int16_t* coef, const uint16_t* q, const double* basis, uint8_t* out,
                        int32_t pw) {
    JPEG_LANES
        if (t == 0) sh.any_ac = 0;
    JPEG_SYNC
    JPEG_LANES
        const int c = coef[t];
        sh.in[(t >> 3) * kRow + (t & 7)] = jpeg_mul((double)c, (double)q[t]);
        JPEG_VOTE_ANY(sh.any_ac, t != 0 && c != 0);
    JPEG_SYNC
    JPEG_LANES  // rows: tmp[v][x] = sum over u of basis[x][u] * in[v][u], from 0.0 in increasing u
        if (sh.any_ac) {
            const int v = t >> 3, x = t & 7;
            double s = 0;
            for (int u = 0; u < 8; ++u) s = jpeg_add(s, jpeg_mul(basis[x * 8 + u], sh.in[v * kRow + u]));
            sh.tmp[v * kRow + x] = s;
        }
    JPEG_SYNC
    JPEG_LANES  // columns: the same over v; level shift, clamp
        int32_t px;
        if (sh.any_ac) {
            const int y = t >> 3, x = t & 7;
            double s = 0;
            for (int v = 0; v < 8; ++v) s = jpeg_add(s, jpeg_mul(basis[y * 8 + v], sh.tmp[v * kRow + x]));
            px = round_to_int(s) + 128;
        } else {
            px = round_to_int(jpeg_mul(sh.in[0], 0.125)) + 128;  // in[0] / 8.0 (exact either way).  The DC-only shortcut: NOT what the two passes give
        }
        sh.px[t] = clamp_u8(px);
    JPEG_SYNC
    JPEG_LANES  // 16 lanes store a dword each
        if (t < 16) {
            uint8_t* dst = out + (int64_t)(t >> 1) * pw + 4 * (t & 1);
#ifdef ME_JPEG_HOST
            memcpy(dst, &sh.px[4 * t], 4);
#else
            *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(&sh.px[4 * t]);
#endif
        }
    JPEG_SYNC
}

// ---- per pixel ---------------------------------------------------------------------------------------------------------------
// Sample (x, y) of the full-resolution plane of component c (Decoder::upsample).  Rows are clamped to the component's own
// height, never the padded one; columns beyond its width are never read.
JPEG_FN int32_t sample_at(const CompDesc& c, const uint8_t* planes, int32_t x, int32_t y) {
    const uint8_t* plane = planes + c.plane_off;
    const int32_t hmax1 = c.height - 1, n = c.width;
    auto row = [&](int32_t r) { return plane + (int64_t)(r < 0 ? 0 : (r > hmax1 ? hmax1 : r)) * c.pw; };
    switch (c.mode) {
        case UP_COPY: return row(y)[x];
        case UP_H2V1: {
            const uint8_t* in = row(y);
            const int32_t i = x >> 1;
            if (x & 1) return i == n - 1 ? in[i] : (in[i] * 3 + in[i + 1] + 2) >> 2;
            return i == 0 ? in[0] : (in[i] * 3 + in[i - 1] + 1) >> 2;
        }
        case UP_H2V2: {
            const int32_t r = y >> 1, i = x >> 1;
            const uint8_t* in0 = row(r);
            const uint8_t* in1 = row((y & 1) ? r + 1 : r - 1);
            const int32_t cur = in0[i] * 3 + in1[i];
            if (x & 1) {
                const int32_t next = i == n - 1 ? cur : in0[i + 1] * 3 + in1[i + 1];
                return (cur * 3 + next + 7) >> 4;
            }
            const int32_t last = i == 0 ? cur : in0[i - 1] * 3 + in1[i - 1];
            return (cur * 3 + last + 8) >> 4;
        }
        case UP_H1V2: {
            const int32_t r = y >> 1;
            const uint8_t* in0 = row(r);
            const uint8_t* in1 = row((y & 1) ? r + 1 : r - 1);
            return (in0[x] * 3 + in1[x] + ((y & 1) ? 2 : 1)) >> 2;
        }
        default: {
            const int32_t i = x / c.fx;
            return row(y / c.fy)[i < n - 1 ? i : n - 1];
        }
    }
}

// libjpeg's ycc_rgb_convert in 16-bit fixed point: the four tables of Decoder::finish as functions of the sample
JPEG_FN void ycc_to_rgb(int32_t y, int32_t cb, int32_t cr, uint8_t* rgb) {
    const int64_t xr = cr - 128, xb = cb - 128;
    const int32_t cr_r = (int32_t)((91881 * xr + 32768) >> 16);    // 1.40200
    const int32_t cb_b = (int32_t)((116130 * xb + 32768) >> 16);   // 1.77200
    const int32_t cr_g = (int32_t)(-46802 * xr);                   // 0.71414
    const int32_t cb_g = (int32_t)(-22554 * xb + 32768);           // 0.34414, with the rounding term
    rgb[0] = clamp_u8(y + cr_r);
    rgb[1] = clamp_u8(y + ((cb_g + cr_g) >> 16));                  // arithmetic shift of a sum that may be negative
    rgb[2] = clamp_u8(y + cb_b);
}

JPEG_FN void pixel_rgb(const Frame& f, const uint8_t* planes, int32_t x, int32_t y, uint8_t* rgb) {
    const int32_t s0 = sample_at(f.comp[0], planes, x, y);
    if (f.color == COLOR_GREY) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)s0;
        return;
    }
    const int32_t s1 = sample_at(f.comp[1], planes, x, y), s2 = sample_at(f.comp[2], planes, x, y);
    if (f.color == COLOR_RGB) {
        rgb[0] = (uint8_t)s0, rgb[1] = (uint8_t)s1, rgb[2] = (uint8_t)s2;
        return;
    }
    ycc_to_rgb(s0, s1, s2, rgb);
}

// where pixel (x, y) of the decoded picture lands in the oriented one (orient.h): its pixel index there
JPEG_FN int64_t oriented_index(const Frame& f, int32_t x, int32_t y) {
    return me_orient::oriented_index(f.width, f.height, x, y, f.orientation);
}

}  // namespace me_jpeg
