// Host check of csrc/orient.h, the one store remap of the JPEG and PNG finish kernels (tests/test_orient_cpu.py).
// For every width and height in 1..9 and every orientation in 0..9 (0 and 9 are orientation 1):
//   - me_orient::oriented_index equals the two functions it replaced, kept below word for word (the JPEG one read its
//     three numbers from a Frame; that struct is cut down to them);
//   - the forwarders of jpeg_recon.h and png_recon.h give the same index;
//   - scattering a numbered picture through it gives exactly apply_orientation's output (host/image_io.cpp, which is
//     written the other way round: the source pixel of an output pixel).
// 1 x N, N x 1 and non-square shapes are where a swapped w / h or an off-by-one in a mirrored axis shows.
#include <cstdint>
#include <cstdio>
#include <vector>

#define ME_JPEG_HOST
#include "../matrix-eyes_amd/csrc/jpeg_recon.h"
#include "../matrix-eyes_amd/csrc/orient.h"
#include "../matrix-eyes_amd/csrc/png_recon.h"
#include "../matrix-eyes_amd/host/image_io.hpp"

namespace before_jpeg {
struct Frame {
    int32_t width, height, orientation;
};
int64_t oriented_index(const Frame& f, int32_t x, int32_t y) {
    const int64_t w = f.width, h = f.height;
    switch (f.orientation) {
        case 2: return (int64_t)y * w + (w - 1 - x);
        case 3: return (h - 1 - y) * w + (w - 1 - x);
        case 4: return (h - 1 - y) * w + x;
        case 5: return (int64_t)x * h + y;
        case 6: return (int64_t)x * h + (h - 1 - y);
        case 7: return (w - 1 - x) * h + (h - 1 - y);
        case 8: return (w - 1 - x) * h + y;
        default: return (int64_t)y * w + x;
    }
}
}  // namespace before_jpeg

namespace before_png {
int64_t oriented_index(int32_t w, int32_t h, int32_t x, int32_t y, int orientation) {
    int64_t ox, oy;
    switch (orientation) {
        case 2: ox = w - 1 - x, oy = y; break;          // flip horizontally
        case 3: ox = w - 1 - x, oy = h - 1 - y; break;  // rotate 180
        case 4: ox = x, oy = h - 1 - y; break;          // flip vertically
        case 5: ox = y, oy = x; break;                  // transpose
        case 6: ox = h - 1 - y, oy = x; break;          // rotate 90 clockwise
        case 7: ox = h - 1 - y, oy = w - 1 - x; break;  // transverse
        case 8: ox = y, oy = w - 1 - x; break;          // rotate 270 clockwise
        default: ox = x, oy = y; break;
    }
    return oy * (orientation >= 5 && orientation <= 8 ? h : w) + ox;
}
}  // namespace before_png

int main() {
    long checked = 0, bad = 0;
    auto expect = [&](bool ok, const char* what, int w, int h, int o, int x, int y) {
        ++checked;
        if (!ok && ++bad <= 20) fprintf(stderr, "%s: %dx%d orientation %d pixel (%d, %d)\n", what, w, h, o, x, y);
    };
    for (int w = 1; w <= 9; ++w)
        for (int h = 1; h <= 9; ++h)
            for (int o = 0; o <= 9; ++o) {
                matrix_eyes::RgbImage img((uint32_t)w, (uint32_t)h);
                for (int i = 0; i < w * h; ++i) img.data[3 * i] = (uint8_t)i, img.data[3 * i + 1] = (uint8_t)(i >> 8), img.data[3 * i + 2] = (uint8_t)o;
                const matrix_eyes::RgbImage want = matrix_eyes::apply_orientation(img, o);
                const bool swap = o >= 5 && o <= 8;
                expect(want.width == (uint32_t)(swap ? h : w) && want.height == (uint32_t)(swap ? w : h), "oriented size", w, h, o, 0, 0);
                std::vector<uint8_t> got(img.data.size(), 0xEE);
                std::vector<int> hits((size_t)w * h, 0);
                me_jpeg::Frame jf{};
                jf.width = w, jf.height = h, jf.orientation = o;
                const me_pngdec::Geom g = me_pngdec::make_geom(w, h, 8, 2, 0);
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const int64_t at = me_orient::oriented_index(w, h, x, y, o);
                        expect(at == before_jpeg::oriented_index(before_jpeg::Frame{w, h, o}, x, y), "the JPEG remap before", w, h, o, x, y);
                        expect(at == before_png::oriented_index(w, h, x, y, o), "the PNG remap before", w, h, o, x, y);
                        expect(at == me_jpeg::oriented_index(jf, x, y), "me_jpeg::oriented_index", w, h, o, x, y);
                        expect(at == me_pngdec::dest_index(g, g.pass[0], x, y, o), "me_pngdec::dest_index", w, h, o, x, y);
                        if (at < 0 || at >= (int64_t)w * h) {
                            expect(false, "index out of the picture", w, h, o, x, y);
                            continue;
                        }
                        ++hits[(size_t)at];
                        for (int c = 0; c < 3; ++c) got[(size_t)at * 3 + c] = img.data[((size_t)y * w + x) * 3 + c];
                    }
                for (int i = 0; i < w * h; ++i) expect(hits[(size_t)i] == 1, "not a permutation", w, h, o, i, 0);
                expect(got == want.data, "scatter differs from apply_orientation", w, h, o, 0, 0);
            }
    printf("%ld checks, %ld failed\n", checked, bad);
    return bad ? 1 : 0;
}
