// The kernels of csrc/jpeg_encode.hip as plain C++: csrc/jpeg_encode.h compiled with ME_JPEG_HOST and run lane by lane in
// the kernels' order, with buffers of exactly the sizes the device path allocates (so the sanitizers see every byte the
// lanes touch).
//   jpeg_encode_host <raw rgb file> <width> <height> <quality> <subsampling 0|1|2> <out.jpg>
// prints "blocks=.. bits=.. stuffed=.. bytes=.." and writes the file.  Exit status 0, 2 on a usage or I/O error.
#define ME_JPEG_HOST
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../matrix-eyes_amd/csrc/jpeg_encode.h"

using namespace me_jpeg_encode;

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: jpeg_encode_host <raw rgb> <w> <h> <quality> <subsampling> <out.jpg>\n");
        return 2;
    }
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), quality = std::atoi(argv[4]), subsampling = std::atoi(argv[5]);
    if (!valid_parameters(w, h, quality, subsampling)) return 2;
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    FILE* in = std::fopen(argv[1], "rb");
    if (!in || std::fread(rgb.data(), 1, rgb.size(), in) != rgb.size()) return 2;
    std::fclose(in);

    std::vector<EncTables> tables(1);
    build_tables(w, h, quality, subsampling, tables[0]);
    const EncCodes& T = tables[0].c;
    const int32_t nblocks = T.d.total_blocks;

    // fdct: workgroups of kFdctBlocks blocks, 8 lanes per block, the transpose through the workgroup's tile
    std::vector<int16_t> coef((size_t)nblocks * 64);
    for (int32_t g = 0; g * kFdctBlocks < nblocks; ++g) {
        std::vector<int32_t> tile((size_t)kFdctBlocks * 8 * kTileStride);
        for (int t = 0; t < kThreads; ++t) {
            const int32_t i = g * kFdctBlocks + t / 8;
            if (i < nblocks) fdct_row_lane(T.d, rgb.data(), i, t % 8, &tile[((size_t)(t / 8) * 8 + t % 8) * kTileStride]);
        }
        for (int t = 0; t < kThreads; ++t) {
            const int32_t i = g * kFdctBlocks + t / 8;
            if (i < nblocks) fdct_col_lane(T, i, t % 8, &tile[(size_t)(t / 8) * 8 * kTileStride], kTileStride, coef.data());
        }
    }
    // bits: one wave per block, then the exclusive sum
    auto mask_of = [&](int32_t i) {
        uint64_t nz = 0;
        for (int k = 0; k < 64; ++k) nz |= (uint64_t)(coef[(size_t)i * 64 + k] != 0) << k;
        return nz;
    };
    std::vector<uint64_t> before((size_t)nblocks + 1, 0);
    for (int32_t i = 0; i < nblocks; ++i) {
        const uint64_t nz = mask_of(i);
        uint32_t sum = 0;
        for (int k = 0; k < 64; ++k) {
            const LaneCode c = lane_code(T, coef.data(), i, k, coef[(size_t)i * 64 + k], nz);
            if (c.len < 0 || c.len > kMaxLaneBits) return 3;
            sum += (uint32_t)c.len;
        }
        before[(size_t)i + 1] = before[(size_t)i] + sum;
    }
    const uint64_t total_bits = before[(size_t)nblocks];
    const int64_t nbytes = (int64_t)((total_bits + 7) / 8);
    const int64_t nchunks = (nbytes + kStuffBytes - 1) / kStuffBytes;
    // pack: the same codes at their offsets, the last block's last lane pads with ones
    std::vector<uint32_t> words((size_t)nchunks * (kStuffBytes / 4), 0);
    for (int32_t i = 0; i < nblocks; ++i) {
        const uint64_t nz = mask_of(i);
        uint64_t at = before[(size_t)i];
        for (int k = 0; k < 64; ++k) {
            const LaneCode c = lane_code(T, coef.data(), i, k, coef[(size_t)i * 64 + k], nz);
            put_bits(words.data(), at, c.bits, c.len);
            at += (uint64_t)c.len;
        }
        if (i == nblocks - 1) {
            const int pad = (int)((8 - (at & 7)) & 7);
            put_bits(words.data(), at, (1ull << pad) - 1ull, pad);
        }
    }
    // stuffing: count, exclusive sum, scatter behind the header
    std::vector<uint64_t> ff((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) ff[(size_t)c + 1] = ff[(size_t)c] + count_ff(words.data(), c);
    const int64_t stuffed = (int64_t)ff[(size_t)nchunks];
    const int32_t hl = T.d.header_len;
    std::vector<uint8_t> file((size_t)(hl + nbytes + stuffed + 2));
    memcpy(file.data(), tables[0].header, (size_t)hl);
    for (int64_t c = 0; c < nchunks; ++c) stuff_chunk(words.data(), nbytes, c, ff[(size_t)c], file.data() + hl);
    file[(size_t)(hl + nbytes + stuffed)] = 0xff, file[(size_t)(hl + nbytes + stuffed) + 1] = 0xd9;

    FILE* out = std::fopen(argv[6], "wb");
    if (!out || std::fwrite(file.data(), 1, file.size(), out) != file.size()) return 2;
    std::fclose(out);
    std::printf("blocks=%d bits=%llu stuffed=%lld bytes=%zu\n", nblocks, (unsigned long long)total_bits, (long long)stuffed, file.size());
    return 0;
}
