// The PNG encoder's per-workgroup routines (matrix-eyes_amd/csrc/png_chunk.h) run on the host, lane by lane:
//   png_chunk_host <rgb file> <width> <height> <png file>
// writes the file the GPU kernels write for that picture (tests/test_png_cpu.py checks it with tests/png_check.py).
#define ME_PNG_HOST 1
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../matrix-eyes_amd/csrc/png_chunk.h"

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s rgb width height png\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    if (w <= 0 || h <= 0) return 2;
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    fclose(f);
    using namespace me_png;
    const int64_t total = ((int64_t)w * 3 + 1) * h, nchunks = (total + kChunk - 1) / kChunk;
    std::vector<uint8_t> stream((size_t)total);
    FilterShared fs;
    for (int row = 0; row < h; ++row) filter_row(fs, rgb.data(), w, row, stream.data());
    std::vector<uint32_t> syms((size_t)kChunk);
    std::vector<uint8_t> slots((size_t)nchunks * kSlot);
    std::vector<ChunkInfo> info((size_t)nchunks);
    auto cs = std::make_unique<ChunkShared>();
    for (int64_t c = 0; c < nchunks; ++c)
        deflate_chunk(*cs, stream.data(), total, (int64_t)w * 3 + 1, c, nchunks, syms.data(), slots.data() + c * kSlot, &info[(size_t)c]);
    std::vector<uint8_t> file((size_t)(kFileSlack + nchunks * (kSlot + 12)));
    std::vector<int64_t> offsets((size_t)nchunks);
    int64_t meta[3];
    layout_file(info.data(), nchunks, w, h, file.data(), offsets.data(), meta);
    GatherShared gs;
    for (int64_t c = 0; c < nchunks; ++c)
        gather_idat(gs, info.data(), slots.data() + c * kSlot, c, nchunks, offsets.data(), meta, file.data());
    if (meta[2] & 2) {
        fprintf(stderr, "a chunk's packed size differs from its estimate\n");
        return 3;
    }
    f = fopen(argv[4], "wb");
    if (!f || fwrite(file.data(), 1, (size_t)meta[0], f) != (size_t)meta[0] || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[4]);
        return 1;
    }
    return 0;
}
