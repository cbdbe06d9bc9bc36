// Host driver of csrc/jpeg_recon.h for tests/test_jpeg_cpu.py: the routines the GPU kernels of csrc/jpeg_decode.hip are made
// of, run lane by lane on the CPU over the host decoder's coefficient interface (decode_jpeg_coefficients), written as a
// PPM.  The test compares the file with `host_selftest decode <in> <out.ppm> oriented` byte for byte.
//
//   jpeg_recon_host <in.jpg> <out.ppm> <orientation 1..8>
// exit 0: written; exit 3: the decoder refused the file (its message on stderr, as the library reports it); 2: usage / I/O
#define ME_JPEG_HOST 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../matrix-eyes_amd/csrc/jpeg_recon.h"
#include "../matrix-eyes_amd/host/image_io.hpp"

using namespace me_jpeg;

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: jpeg_recon_host <in.jpg> <out.ppm> <orientation>\n");
        return 2;
    }
    const int orientation = std::atoi(argv[3]);
    if (orientation < 1 || orientation > 8) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    matrix_eyes::JpegCoefficients c;
    try {
        c = matrix_eyes::decode_jpeg_coefficients(file, "<jpeg>");
        matrix_eyes::check_jpeg_reconstructible(c, "<jpeg>");
    } catch (const matrix_eyes::ImageError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    // the plan of jpeg_decode.hip (plan()), restated
    Frame f;
    IdctTables tab;
    std::memset(&f, 0, sizeof(f));
    std::memset(&tab, 0, sizeof(tab));
    f.width = c.width, f.height = c.height, f.ncomp = (int32_t)c.comps.size(), f.orientation = orientation;
    int64_t coef_off = 0, plane_off = 0;
    int32_t block0 = 0;
    for (int i = 0; i < f.ncomp; ++i) {
        const matrix_eyes::JpegComponent& k = c.comps[(size_t)i];
        CompDesc& d = f.comp[i];
        d.width = k.width, d.height = k.height, d.blocks_w = k.blocks_w, d.blocks_h = k.blocks_h, d.pw = k.blocks_w * 8;
        d.fx = c.hmax / k.h, d.fy = c.vmax / k.v;
        const int n = k.width;
        d.mode = d.fx == 1 && d.fy == 1 ? UP_COPY
                 : d.fx == 2 && d.fy == 1 && n > 2 ? UP_H2V1
                 : d.fx == 2 && d.fy == 2 && n > 2 ? UP_H2V2
                 : d.fx == 1 && d.fy == 2 ? UP_H1V2 : UP_REPL;
        d.block0 = block0, d.qsel = i, d.coef_off = coef_off, d.plane_off = plane_off;
        const int64_t blocks = (int64_t)k.blocks_w * k.blocks_h;
        block0 += (int32_t)blocks, coef_off += blocks * 64, plane_off += blocks * 64;
        for (int j = 0; j < 64; ++j) tab.q[i][j] = c.qt[k.tq][j];
    }
    f.total_blocks = block0;
    const bool rgb = f.ncomp == 3 && (c.adobe_transform == 0 || (c.adobe_transform < 0 && c.comps[0].id == 'R' &&
                                                                 c.comps[1].id == 'G' && c.comps[2].id == 'B'));
    f.color = f.ncomp == 1 ? COLOR_GREY : (rgb ? COLOR_RGB : COLOR_YCC);
    matrix_eyes::jpeg_idct_basis(tab.basis);

    // jpeg_idct_kernel, block by block.  The planes start as 0xAA: a sample the finish pass must not read stays visible
    std::vector<uint8_t> planes((size_t)plane_off, 0xAA);
    const int16_t* coef = c.comps[0].coef;  // the components' coefficients are contiguous, in component order
    BlockShared sh;
    for (int blk = 0; blk < f.total_blocks; ++blk) {
        int ci = 0;
        if (f.ncomp == 3) ci = blk >= f.comp[2].block0 ? 2 : (blk >= f.comp[1].block0 ? 1 : 0);
        const CompDesc& d = f.comp[ci];
        const int lb = blk - d.block0, by = lb / d.blocks_w, bx = lb - by * d.blocks_w;
        idct_block(sh, true, coef + d.coef_off + (int64_t)lb * 64, tab.q[ci], tab.basis,
                   planes.data() + d.plane_off + (int64_t)by * 8 * d.pw + (int64_t)bx * 8, d.pw);
    }
    // jpeg_finish_kernel, pixel by pixel
    const bool swap = orientation >= 5;
    const int ow = swap ? f.height : f.width, oh = swap ? f.width : f.height;
    std::vector<uint8_t> out((size_t)ow * oh * 3, 0);
    for (int y = 0; y < f.height; ++y)
        for (int x = 0; x < f.width; ++x) pixel_rgb(f, planes.data(), x, y, &out[(size_t)oriented_index(f, x, y) * 3]);
    std::ofstream o(argv[2], std::ios::binary);
    o << "P6\n" << ow << " " << oh << "\n255\n";
    if (!o.write((const char*)out.data(), (std::streamsize)out.size())) return 2;
    return 0;
}
