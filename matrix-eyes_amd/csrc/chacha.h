// The keyed noise of the stereogram: a ChaCha block function addressed by position, the pixel addressing
// on top of it and the expansion of a 64-bit seed into a key.  One text for the kernels (stereogram_noise.hip), the host twin
// behind me_stereogram_noise_host and the stand-alone program tests/chacha_host.cpp.  Plain C++, integer arithmetic only.
//
// The definition is this project's own.  It is modelled on the ChaCha12 block generator and the PCG32 seed expansion that
// common random-number libraries use, and claims parity with none of them.
#ifndef ME_CHACHA_H
#define ME_CHACHA_H
#include <stdint.h>

#ifdef __HIPCC__
#define ME_CHACHA_HD __host__ __device__
#else
#define ME_CHACHA_HD
#endif

namespace me_chacha {

constexpr int kNoiseRounds = 12;  // the library's stream; 20 exists for the cross-check against other implementations

// the eight little-endian key words, as they travel in a kernel's arguments
struct Key {
    uint32_t w[8];
};

ME_CHACHA_HD inline uint32_t rotl32(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

#define ME_CHACHA_QR(a, b, c, d)                  \
    a += b, d ^= a, d = me_chacha::rotl32(d, 16); \
    c += d, b ^= c, b = me_chacha::rotl32(b, 12); \
    a += b, d ^= a, d = me_chacha::rotl32(d, 8);  \
    c += d, b ^= c, b = me_chacha::rotl32(b, 7);

// Block `counter` of the key's stream: words 0..3 "expand 32-byte k", 4..11 the key, 12 / 13 the counter's halves, 14 / 15
// zero; ROUNDS / 2 double rounds (column, then diagonal); the input state added at the end.
template <int ROUNDS>
ME_CHACHA_HD inline void block(const Key& key, uint64_t counter, uint32_t out[16]) {
    static_assert(ROUNDS > 0 && ROUNDS % 2 == 0, "whole double rounds");
    const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
    const uint32_t n0 = (uint32_t)counter, n1 = (uint32_t)(counter >> 32);
    uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3;
    uint32_t x4 = key.w[0], x5 = key.w[1], x6 = key.w[2], x7 = key.w[3];
    uint32_t x8 = key.w[4], x9 = key.w[5], x10 = key.w[6], x11 = key.w[7];
    uint32_t x12 = n0, x13 = n1, x14 = 0, x15 = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < ROUNDS; r += 2) {
        ME_CHACHA_QR(x0, x4, x8, x12)
        ME_CHACHA_QR(x1, x5, x9, x13)
        ME_CHACHA_QR(x2, x6, x10, x14)
        ME_CHACHA_QR(x3, x7, x11, x15)
        ME_CHACHA_QR(x0, x5, x10, x15)
        ME_CHACHA_QR(x1, x6, x11, x12)
        ME_CHACHA_QR(x2, x7, x8, x13)
        ME_CHACHA_QR(x3, x4, x9, x14)
    }
    out[0] = x0 + c0, out[1] = x1 + c1, out[2] = x2 + c2, out[3] = x3 + c3;
    out[4] = x4 + key.w[0], out[5] = x5 + key.w[1], out[6] = x6 + key.w[2], out[7] = x7 + key.w[3];
    out[8] = x8 + key.w[4], out[9] = x9 + key.w[5], out[10] = x10 + key.w[6], out[11] = x11 + key.w[7];
    out[12] = x12 + n0, out[13] = x13 + n1, out[14] = x14, out[15] = x15;
}
#undef ME_CHACHA_QR

// ---- pixel addressing: pixel i = y * out_w + x takes keystream word i, which is word i & 15 of block i >> 4 ------------
ME_CHACHA_HD inline uint64_t pixel_index(int64_t y, int64_t out_w, int64_t x) { return (uint64_t)(y * out_w + x); }
ME_CHACHA_HD inline uint64_t pixel_block(uint64_t i) { return i >> 4; }
ME_CHACHA_HD inline int pixel_lane(uint64_t i) { return (int)(i & 15); }
// R, G, B are bits 0-7, 8-15 and 16-23 of the word; the top byte is dropped
ME_CHACHA_HD inline void word_to_rgb(uint32_t w, uint8_t* rgb) {
    rgb[0] = (uint8_t)w, rgb[1] = (uint8_t)(w >> 8), rgb[2] = (uint8_t)(w >> 16);
}
// four consecutive words' twelve bytes as three little-endian dwords
ME_CHACHA_HD inline void pack_rgb4(const uint32_t w[4], uint32_t d[3]) {
    d[0] = (w[0] & 0xffffffu) | (w[1] << 24);
    d[1] = ((w[1] >> 8) & 0xffffu) | (w[2] << 16);
    d[2] = ((w[2] >> 16) & 0xffu) | (w[3] << 8);
}

ME_CHACHA_HD inline Key key_from_bytes(const uint8_t key[32]) {
    Key k;
    for (int i = 0; i < 8; ++i)
        k.w[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 | (uint32_t)key[4 * i + 3] << 24;
    return k;
}

// seed -> key: eight steps of a 64-bit LCG, each giving one xorshift-rotate output as four little-endian bytes
ME_CHACHA_HD inline void key_from_seed(uint64_t seed, uint8_t key[32]) {
    const uint64_t MUL = 6364136223846793005ull, INC = 11634580027462260723ull;
    uint64_t state = seed;
    for (int i = 0; i < 8; ++i) {
        state = state * MUL + INC;
        const uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27);
        const int rot = (int)(state >> 59);
        const uint32_t v = (xs >> rot) | (xs << ((32 - rot) & 31));
        key[4 * i] = (uint8_t)v, key[4 * i + 1] = (uint8_t)(v >> 8), key[4 * i + 2] = (uint8_t)(v >> 16), key[4 * i + 3] = (uint8_t)(v >> 24);
    }
}

// The host twin of the fill kernel: u8 [out_h, out_w, 3], block by block on the calling thread
inline void noise_fill_host(const uint8_t key_bytes[32], int64_t out_w, int64_t out_h, uint8_t* out) {
    const Key key = key_from_bytes(key_bytes);
    const uint64_t pixels = (uint64_t)(out_w * out_h);
    uint32_t words[16];
    for (uint64_t b = 0; b * 16 < pixels; ++b) {
        block<kNoiseRounds>(key, b, words);
        const uint64_t n = pixels - b * 16 < 16 ? pixels - b * 16 : 16;
        for (uint64_t k = 0; k < n; ++k) word_to_rgb(words[k], out + 3 * (b * 16 + k));
    }
}

}  // namespace me_chacha
#endif  // ME_CHACHA_H
