// Reconstruction of a PNG picture from its filtered stream (filter byte + row, pass after pass), as host/png_decoder.cpp
// does it and byte for byte: the scanline filters, the Adam7 pass geometry, the conversion of every (colour type, depth)
// pair to 8-bit RGB the way the reference's decoder stack does it (into_rgb8) and the EXIF orientation as a remap of the
// store address.  Plain inline routines with no HIP call in them: the host decoder, the kernels of csrc/png_decode.hip and
// the plain-C++ driver of the CPU tests (tests/png_recon_host.cpp) are all made of them.
#pragma once
#include <stdint.h>

#include "orient.h"

#if defined(__HIPCC__)
#define PNGDEC_FN __host__ __device__ inline
#else
#define PNGDEC_FN inline
#endif

namespace me_pngdec {

constexpr int kMaxPasses = 7;

struct Pass {
    int32_t x0, y0, dx, dy;      // picture pixel of pass pixel (px, py): (x0 + px * dx, y0 + py * dy)
    int32_t pw, ph;              // pixels of the pass (either may be 0: the pass is not in the stream)
    int32_t stride;              // bytes of one row without its filter byte
    int32_t pad;
    int64_t offset;              // of the pass's first filter byte in the filtered stream
};
struct Geom {
    int32_t width, height;       // of the decoded picture, before the orientation
    int32_t depth, ctype, interlace;
    int32_t channels, bits_pp;
    int32_t bpp;                 // the filters' "corresponding byte" distance: max(1, bits_pp / 8)
    int32_t npass;               // 1 or 7
    int32_t pad;
    int64_t total;               // bytes of the filtered stream
    Pass pass[kMaxPasses];
};

// channels of a colour type; 0: not a colour type
PNGDEC_FN int channels_of(int ctype) { return ctype == 0 || ctype == 3 ? 1 : ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0; }

// Adam7 pass `ps` (0..6) as (x0, y0, dx, dy)
PNGDEC_FN void adam7_pass(int ps, int32_t* x0, int32_t* y0, int32_t* dx, int32_t* dy) {
    // {0,0,8,8} {4,0,8,8} {0,4,4,8} {2,0,4,4} {0,2,2,4} {1,0,2,2} {0,1,1,2}
    *x0 = ps == 1 ? 4 : ps == 3 ? 2 : ps == 5 ? 1 : 0;
    *y0 = ps == 2 ? 4 : ps == 4 ? 2 : ps == 6 ? 1 : 0;
    *dx = ps < 2 ? 8 : ps < 4 ? 4 : ps < 6 ? 2 : 1;
    *dy = ps < 3 ? 8 : ps < 5 ? 4 : 2;
}

// the pass (0..6) that holds picture pixel (x, y) of an interlaced file
PNGDEC_FN int adam7_pass_of(int32_t x, int32_t y) {
    const int xs = x & 7, ys = y & 7;
    if (ys & 1) return 6;
    if (xs & 1) return 5;
    if (ys & 2) return 4;
    if (xs & 2) return 3;
    if (ys & 4) return 2;
    return (xs & 4) ? 1 : 0;
}

// a non-interlaced picture is one pass over every pixel
PNGDEC_FN Geom make_geom(int32_t width, int32_t height, int depth, int ctype, int interlace) {
    Geom g;
    g.width = width, g.height = height, g.depth = depth, g.ctype = ctype, g.interlace = interlace;
    g.channels = channels_of(ctype), g.bits_pp = g.channels * depth;
    g.bpp = g.bits_pp >= 8 ? g.bits_pp / 8 : 1;
    g.npass = interlace ? 7 : 1, g.pad = 0;
    int64_t total = 0;
    for (int ps = 0; ps < kMaxPasses; ++ps) {
        Pass& p = g.pass[ps];
        p.x0 = p.y0 = 0, p.dx = p.dy = 1, p.pw = p.ph = 0, p.stride = 0, p.pad = 0, p.offset = total;
        if (ps >= g.npass) continue;
        if (interlace) adam7_pass(ps, &p.x0, &p.y0, &p.dx, &p.dy);
        p.pw = (int32_t)(((int64_t)width + p.dx - 1 - p.x0) / p.dx);
        p.ph = (int32_t)(((int64_t)height + p.dy - 1 - p.y0) / p.dy);
        p.stride = (int32_t)(((int64_t)p.pw * g.bits_pp + 7) / 8);
        if (p.pw && p.ph) total += ((int64_t)p.stride + 1) * p.ph;
    }
    g.total = total;
    return g;
}

PNGDEC_FN int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// one reconstruction step: x the filtered byte, a the byte `bpp` to the left, b the byte above, c the one above a
// (zeros outside the row and above the first row of a pass).  A filter above 4 is the caller's to refuse.
PNGDEC_FN uint8_t recon(int filter, int x, int a, int b, int c) {
    switch (filter) {
        case 1: x += a; break;
        case 2: x += b; break;
        case 3: x += (a + b) / 2; break;
        case 4: x += paeth(a, b, c); break;
        default: break;
    }
    return (uint8_t)x;
}

// channel c of pixel x of a reconstructed row, depth 8 or 16: 16-bit samples rounded as (v + 128) / 257
PNGDEC_FN int sample8(const Geom& g, const uint8_t* row, int32_t x, int c) {
    if (g.depth == 8) return row[(int64_t)x * g.channels + c];
    const uint8_t* p = row + ((int64_t)x * g.channels + c) * 2;
    return (((int)p[0] << 8 | p[1]) + 128) / 257;
}

// depth < 8: one channel, big-endian bit order
PNGDEC_FN int packed_sample(const Geom& g, const uint8_t* row, int32_t x) {
    const int64_t bit = (int64_t)x * g.depth;
    return (row[bit >> 3] >> (8 - g.depth - (int)(bit & 7))) & ((1 << g.depth) - 1);
}

// pixel px of a reconstructed row as 8-bit RGB: grey of 1 / 2 / 4 bits scaled to the full range (x255, x85, x17), grey
// to RGB, alpha dropped, the palette looked up.  False: the palette index is out of range (3 * index + 2 >= plte_bytes).
PNGDEC_FN bool pixel_rgb(const Geom& g, const uint8_t* row, int32_t px, const uint8_t* plte, int32_t plte_bytes, uint8_t* out) {
    switch (g.ctype) {
        case 0: {
            const int grey_scale = g.depth < 8 ? 255 / ((1 << g.depth) - 1) : 1;
            out[0] = out[1] = out[2] = (uint8_t)(g.depth < 8 ? packed_sample(g, row, px) * grey_scale : sample8(g, row, px, 0));
            return true;
        }
        case 4: out[0] = out[1] = out[2] = (uint8_t)sample8(g, row, px, 0); return true;
        case 3: {
            const int32_t k = (g.depth < 8 ? packed_sample(g, row, px) : row[px]) * 3;
            if (k + 2 >= plte_bytes) return false;
            out[0] = plte[k], out[1] = plte[k + 1], out[2] = plte[k + 2];
            return true;
        }
        default:
            out[0] = (uint8_t)sample8(g, row, px, 0), out[1] = (uint8_t)sample8(g, row, px, 1);
            out[2] = (uint8_t)sample8(g, row, px, 2);
            return true;
    }
}

using me_orient::oriented_index;   // orient.h: where picture pixel (x, y) goes under apply_orientation(orientation)

// the destination pixel of pass pixel (px, py) under orientation 1..8
PNGDEC_FN int64_t dest_index(const Geom& g, const Pass& p, int32_t px, int32_t py, int orientation) {
    return oriented_index(g.width, g.height, p.x0 + px * p.dx, p.y0 + py * p.dy, orientation);
}

// de-interlacing the other way round: the pass and the pass pixel that hold picture pixel (x, y)
PNGDEC_FN int pass_pixel(const Geom& g, int32_t x, int32_t y, int32_t* px, int32_t* py) {
    if (!g.interlace) {
        *px = x, *py = y;
        return 0;
    }
    const int ps = adam7_pass_of(x, y);
    int32_t x0, y0, dx, dy;
    adam7_pass(ps, &x0, &y0, &dx, &dy);
    *px = (x - x0) / dx, *py = (y - y0) / dy;
    return ps;
}

// the rows [*py0, *py1) of pass p that lie in picture rows [y_begin, y_end): one band of the unfilter kernel
PNGDEC_FN void band_rows_of(const Pass& p, int64_t y_begin, int64_t y_end, int32_t* py0, int32_t* py1) {
    const int64_t a = y_begin > p.y0 ? (y_begin - p.y0 + p.dy - 1) / p.dy : 0;
    const int64_t b = y_end > p.y0 ? (y_end - p.y0 + p.dy - 1) / p.dy : 0;
    *py0 = (int32_t)(a < p.ph ? a : p.ph), *py1 = (int32_t)(b < p.ph ? b : p.ph);
    if (!p.pw) *py0 = *py1 = 0;
}

// The skewed wavefront of the unfilter kernel, one step of one lane: the lane owns a row; at every step it takes the byte
// group (one pixel's `BPP` bytes) its upper neighbour made one step earlier as b, keeps its own b of the step before as c
// and its own result of the step before as a.
template <int BPP>
struct LaneState {
    uint8_t a[BPP];   // this row, one pixel to the left
    uint8_t b[BPP];   // the row above, this pixel (after step())
};
template <int BPP>
PNGDEC_FN void lane_reset(LaneState<BPP>& s) {
    for (int k = 0; k < BPP; ++k) s.a[k] = 0, s.b[k] = 0;
}
// above[]: the reconstructed pixel of the row above at this position; x[] in: filtered, out: reconstructed
template <int BPP>
PNGDEC_FN void lane_step(LaneState<BPP>& s, int filter, const uint8_t* above, uint8_t* x) {
    for (int k = 0; k < BPP; ++k) {
        const int c = s.b[k];
        s.b[k] = above[k];
        x[k] = recon(filter, x[k], s.a[k], s.b[k], c);
        s.a[k] = x[k];
    }
}

}  // namespace me_pngdec
