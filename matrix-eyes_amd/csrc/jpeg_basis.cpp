// The basis of the JPEG decoder's separable IDCT (T.81 A.3.3): basis[x][u] = C(u) / 2 * cos((2x + 1) u pi / 16).
//
// Plain C++, compiled by g++ with -ffp-contract=off (Makefile), and the ONLY place the 64 doubles are computed: the host
// decoder (host/jpeg_decoder.cpp idct_all) and the device decoder (jpeg_decode.hip, which passes the table to its kernel)
// both call it, so the two reconstruct from the same bits -- the device's cos is another function.
#include <cmath>

#include "../host/image_io.hpp"

namespace matrix_eyes {

void jpeg_idct_basis(double basis[64]) {
    for (int x = 0; x < 8; ++x)
        for (int u = 0; u < 8; ++u)
            basis[x * 8 + u] = (u == 0 ? std::sqrt(0.125) : 0.5) * std::cos((2 * x + 1) * u * 3.14159265358979323846 / 16.0);
}

}  // namespace matrix_eyes
