// Stand-alone driver of csrc/chacha.h for tests/test_stereogram_noise_cpu.py (plain C++, built with the sanitizers):
//   chacha_host <key: 64 hex digits>
// prints, for the key,
//   block <rounds> <counter> <128 hex digits>     counters 0, 1, 2^32 - 1, 2^32, 2^32 + 1 at 12 and 20 rounds
//   seed <seed> <64 hex digits>                   the keys of the seeds 0, 99 and 2^64 - 1
//   noise <out_w> <out_h> <hex of out_h * out_w * 3 bytes>   the host twin at 17 x 2 and 5 x 3, into exactly-sized buffers
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../matrix-eyes_amd/csrc/chacha.h"

static void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

template <int ROUNDS>
static void print_block(const me_chacha::Key& key, uint64_t counter) {
    uint32_t words[16];
    me_chacha::block<ROUNDS>(key, counter, words);
    uint8_t bytes[64];
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 4; ++k) bytes[4 * i + k] = (uint8_t)(words[i] >> (8 * k));
    std::printf("block %d %" PRIu64 " ", ROUNDS, counter);
    print_hex(bytes, 64);
}

int main(int argc, char** argv) {
    uint8_t key_bytes[32] = {0};
    if (argc > 1) {
        if (std::strlen(argv[1]) != 64) return 2;
        for (int i = 0; i < 32; ++i) {
            unsigned v = 0;
            if (std::sscanf(argv[1] + 2 * i, "%2x", &v) != 1) return 2;
            key_bytes[i] = (uint8_t)v;
        }
    }
    const me_chacha::Key key = me_chacha::key_from_bytes(key_bytes);
    const uint64_t counters[5] = {0, 1, 0xffffffffull, 0x100000000ull, 0x100000001ull};
    for (uint64_t c : counters) print_block<12>(key, c);
    for (uint64_t c : counters) print_block<20>(key, c);
    const uint64_t seeds[3] = {0, 99, ~0ull};
    for (uint64_t s : seeds) {
        uint8_t k[32];
        me_chacha::key_from_seed(s, k);
        std::printf("seed %" PRIu64 " ", s);
        print_hex(k, 32);
    }
    const int sizes[2][2] = {{17, 2}, {5, 3}};
    for (const auto& wh : sizes) {
        std::vector<uint8_t> out((size_t)wh[0] * wh[1] * 3);
        me_chacha::noise_fill_host(key_bytes, wh[0], wh[1], out.data());
        std::printf("noise %d %d ", wh[0], wh[1]);
        print_hex(out.data(), out.size());
    }
    return 0;
}
