// The EXIF orientation as a remap of the store address: where pixel (x, y) of a decoded w x h picture lands under
// apply_orientation(orientation) of host/image_io.cpp -- its pixel index in the oriented picture, whose width is h for
// orientations 5..8 and w otherwise.  Any other value is orientation 1.  Shared by the JPEG and PNG finish kernels
// (jpeg_recon.h, png_recon.h) and their host drivers; apply_orientation itself is written the other way round (the source
// pixel of an output pixel) and stays the independent yardstick (tests/orient_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ME_ORIENT_FN __host__ __device__ inline
#else
#define ME_ORIENT_FN inline
#endif

namespace me_orient {

ME_ORIENT_FN int64_t oriented_index(int32_t w, int32_t h, int32_t x, int32_t y, int orientation) {
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

}  // namespace me_orient
