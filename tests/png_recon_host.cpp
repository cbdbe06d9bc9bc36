// Host driver of csrc/png_recon.h for tests/test_png_decode_cpu.py: the routines the GPU kernels of csrc/png_decode.hip are
// made of, run lane by lane on the CPU in the kernels' own order -- bands, row groups of 64 lanes, tiles of the LDS size,
// the skewed diagonal with the value of the lane above taken from one step earlier -- over the host decoder's
// parse_png_header / inflate_png, written as a PPM.  The test compares the file with
// `host_selftest decode <in> <out.ppm> oriented` byte for byte.
//
//   png_recon_host <in.png> <out.ppm> <orientation 1..8> [band_rows]
// exit 0: written; exit 3: the decoder refused the file (its message on stderr, as the library reports it); 2: usage / I/O
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../matrix-eyes_amd/csrc/png_recon.h"
#include "../matrix-eyes_amd/host/image_io.hpp"

using namespace me_pngdec;

namespace {

constexpr int kWaves = 4, kGroupRows = 64, kTileBytes = 216;   // csrc/png_decode.hip

// png_unfilter_kernel<BPP>, one workgroup (= one pass of one band), in place
template <int BPP>
void unfilter_pass(const Pass& p, int r0, int r1, uint8_t* stream) {
    constexpr int kPitch = kTileBytes + BPP + 4;
    if (r0 >= r1) return;
    const int64_t row_pitch = (int64_t)p.stride + 1;
    const int ngroups = (r1 - r0 + kGroupRows - 1) / kGroupRows;
    const int ntiles = (p.stride + kTileBytes - 1) / kTileBytes;
    std::vector<uint8_t> tiles((size_t)kWaves * (kGroupRows + 1) * kPitch);
    for (int round = 0; round * kWaves < ngroups; ++round) {
        LaneState<BPP> st[kWaves][64];
        int filter[kWaves][64];
        for (int wave = 0; wave < kWaves; ++wave)
            for (int lane = 0; lane < 64; ++lane) {
                lane_reset(st[wave][lane]);
                const int group = round * kWaves + wave, row0 = r0 + group * kGroupRows;
                const int nrows = group < ngroups ? std::min(kGroupRows, r1 - row0) : 0;
                filter[wave][lane] = lane < nrows ? stream[p.offset + (int64_t)(row0 + lane) * row_pitch] : 0;
            }
        for (int s = 0; s < ntiles + kWaves - 1; ++s)
            for (int wave = 0; wave < kWaves; ++wave) {
                const int group = round * kWaves + wave, row0 = r0 + group * kGroupRows;
                const int nrows = group < ngroups ? std::min(kGroupRows, r1 - row0) : 0;
                const int k = s - wave;
                if (!(nrows > 0 && k >= 0 && k < ntiles)) continue;
                const int xb = k * kTileBytes, tb = std::min(kTileBytes, p.stride - xb), npx = tb / BPP;
                uint8_t* tile = &tiles[(size_t)wave * (kGroupRows + 1) * kPitch];
                std::memset(tile, 0xAA, (size_t)(kGroupRows + 1) * kPitch);   // what the walk must not read stays visible
                for (int c = 0; c < tb; ++c) tile[c] = row0 > 0 ? stream[p.offset + (int64_t)(row0 - 1) * row_pitch + 1 + xb + c] : 0;
                for (int r = 0; r < nrows; ++r)
                    std::memcpy(tile + (r + 1) * kPitch, &stream[p.offset + (int64_t)(row0 + r) * row_pitch + 1 + xb], (size_t)tb);
                for (int t = 0; t < npx + nrows - 1; ++t) {
                    uint8_t up[64][BPP];   // the cross-lane move: every lane's last result, shifted one lane down
                    for (int lane = 1; lane < 64; ++lane) std::memcpy(up[lane], st[wave][lane - 1].a, BPP);
                    for (int lane = 0; lane < nrows; ++lane) {
                        const int px = t - lane;
                        if (px < 0 || px >= npx) continue;
                        uint8_t* my_row = tile + (lane + 1) * kPitch;
                        lane_step<BPP>(st[wave][lane], filter[wave][lane], lane == 0 ? tile + px * BPP : up[lane], my_row + px * BPP);
                    }
                }
                for (int r = 0; r < nrows; ++r)
                    std::memcpy(&stream[p.offset + (int64_t)(row0 + r) * row_pitch + 1 + xb], tile + (r + 1) * kPitch, (size_t)tb);
            }
    }
}

void unfilter_band(const Geom& g, int64_t y_begin, int64_t y_end, uint8_t* stream) {
    for (int ps = 0; ps < g.npass; ++ps) {
        int32_t r0, r1;
        band_rows_of(g.pass[ps], y_begin, y_end, &r0, &r1);
        switch (g.bpp) {
            case 1: unfilter_pass<1>(g.pass[ps], r0, r1, stream); break;
            case 2: unfilter_pass<2>(g.pass[ps], r0, r1, stream); break;
            case 3: unfilter_pass<3>(g.pass[ps], r0, r1, stream); break;
            case 4: unfilter_pass<4>(g.pass[ps], r0, r1, stream); break;
            case 6: unfilter_pass<6>(g.pass[ps], r0, r1, stream); break;
            default: unfilter_pass<8>(g.pass[ps], r0, r1, stream); break;
        }
    }
}

// the device path's answer to a defect: the host decoder runs whole and its words stand
int refuse_as_the_host(const std::vector<uint8_t>& file) {
    try {
        (void)matrix_eyes::decode_png(file, "<png>", nullptr);
    } catch (const matrix_eyes::ImageError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::fprintf(stderr, "the driver refused a file the host decoder accepts\n");
    return 4;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4 && argc != 5) {
        std::fprintf(stderr, "usage: png_recon_host <in.png> <out.ppm> <orientation> [band_rows]\n");
        return 2;
    }
    const int orientation = std::atoi(argv[3]);
    const int band_rows = argc == 5 ? std::atoi(argv[4]) : kWaves * kGroupRows;
    if (orientation < 1 || orientation > 8 || band_rows < 1) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    matrix_eyes::PngFrame f;
    std::vector<uint8_t> stream;
    try {
        f = matrix_eyes::parse_png_header(file, "<png>");
        stream.resize(f.total);
        matrix_eyes::inflate_png(f, file, "<png>", stream.data());
    } catch (const matrix_eyes::ImageError& e) {
        const int rc = refuse_as_the_host(file);   // the same words, by the way the device path gets them
        return rc;
    }
    const Geom& g = f.geom;
    for (int ps = 0; ps < g.npass; ++ps)
        for (int32_t py = 0; g.pass[ps].pw && py < g.pass[ps].ph; ++py)
            if (stream[g.pass[ps].offset + (int64_t)py * ((int64_t)g.pass[ps].stride + 1)] > 4) return refuse_as_the_host(file);
    for (int64_t y = 0; y < g.height; y += band_rows) unfilter_band(g, y, std::min<int64_t>(g.height, y + band_rows), stream.data());

    // png_finish_kernel, pixel by pixel in picture order
    const bool swap = orientation >= 5;
    const int64_t ow = swap ? g.height : g.width, oh = swap ? g.width : g.height;
    std::vector<uint8_t> out((size_t)(ow * oh * 3), 0);
    for (int32_t y = 0; y < g.height; ++y)
        for (int32_t x = 0; x < g.width; ++x) {
            int32_t px, py;
            const Pass& p = g.pass[pass_pixel(g, x, y, &px, &py)];
            const uint8_t* row = stream.data() + p.offset + (int64_t)py * ((int64_t)p.stride + 1) + 1;
            if (!pixel_rgb(g, row, px, f.plte.data(), (int32_t)std::min<size_t>(f.plte.size(), 768),
                           &out[(size_t)dest_index(g, p, px, py, orientation) * 3]))
                return refuse_as_the_host(file);
        }
    std::ofstream o(argv[2], std::ios::binary);
    o << "P6\n" << ow << " " << oh << "\n255\n";
    if (!o.write((const char*)out.data(), (std::streamsize)out.size())) return 2;
    return 0;
}
