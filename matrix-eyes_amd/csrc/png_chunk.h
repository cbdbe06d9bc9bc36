// The per-workgroup routines of the PNG encoder (png_encode.hip): the row filter, one deflate chunk, the file layout
// and the gather of one IDAT.  Written as a sequence of PHASES -- PNG_LANES { code of lane t } PNG_SYNC -- with every
// value that lives across a phase kept in the workgroup's shared struct, so that the same text is a HIP kernel body
// (a phase = the code of thread t, PNG_SYNC = __syncthreads) and, with ME_PNG_HOST defined, plain C++ that runs a
// phase lane by lane (tests/png_chunk_host.cpp: the encoder's logic is checked against zlib without a GPU).
//
// The stream format is pigz's: the filtered picture is cut into chunks of kPngChunk bytes, every chunk is one dynamic
// Huffman block (or stored blocks when that is shorter) that ends byte-aligned behind an empty stored block, matches
// may reach back into the preceding chunk's INPUT (the decoder's window is continuous), so chunks are independent.
// Everything is a pure function of the input: integer atomics only (max, add, or), whose results do not depend on order.
#pragma once
#include <stdint.h>
#include <string.h>
#ifndef ME_PNG_HOST
#include "scan.h"
#endif

namespace me_png {

constexpr int kThreads = 256;
constexpr int kChunk = 65536;        // bytes of filtered stream per workgroup / deflate block / IDAT
constexpr int kWindow = 8192;        // history primed from the preceding chunk's input (>= 4 KiB: a stereogram row repeats at <= 1.5 KB)
constexpr int kMaxDist = 32768;
constexpr int kMinMatch = 4, kMaxMatch = 258;   // the hash covers 4 bytes: a 3-byte match at these distances costs more than 3 literals
constexpr int kHashBits = 12;       // per table; two tables (4-byte and 8-byte contexts) of 2^12 entries = 32 KiB of LDS
constexpr int kLazyBelow = 32;      // a match shorter than this yields to a longer one starting at the next byte
constexpr int kSlot = kChunk + 64;   // worst case of one chunk: stored, 2 blocks * 5 bytes of header
constexpr int kStageWords = 448;     // 7 carried bits + 256 symbols * 48 bits, + the words a shifted symbol spills into
constexpr int kFileHead = 33;        // signature + IHDR
constexpr int kFileSlack = 64;       // signature, IHDR, zlib header, Adler-32, IEND

struct ChunkInfo {
    uint32_t nbytes;     // deflate bytes in the chunk's slot
    uint32_t adler_a;    // sum of the chunk's bytes mod 65521
    uint32_t adler_b;    // sum of (n - i) * byte[i] mod 65521
    uint32_t flags;      // bit 0: stored; bit 1: the size estimate and the packed size disagree (never expected)
};

#ifdef ME_PNG_HOST
#define PNG_FN inline
#define PNG_LANES for (int t = 0; t < ::me_png::kThreads; ++t) {
#define PNG_SYNC }
template <class T> inline void lds_max(T* p, T v) { if (v > *p) *p = v; }
template <class T> inline void lds_add(T* p, T v) { *p += v; }
template <class T> inline void lds_or(T* p, T v) { *p |= v; }
#else
#define PNG_FN __device__ inline
#define PNG_LANES { const int t = (int)threadIdx.x;
#define PNG_SYNC } __syncthreads();
template <class T> __device__ inline void lds_max(T* p, T v) { atomicMax(p, v); }
template <class T> __device__ inline void lds_add(T* p, T v) { atomicAdd(p, v); }
template <class T> __device__ inline void lds_or(T* p, T v) { atomicOr(p, v); }
#endif

// ---- CRC-32 (reflected, polynomial 0xEDB88320), with zlib's crc32_combine arithmetic ------------------------------------
PNG_FN uint32_t crc_table_entry(uint32_t n) {
    for (int k = 0; k < 8; ++k) n = (n & 1) ? (n >> 1) ^ 0xEDB88320u : n >> 1;
    return n;
}
// a * b mod P in the reflected representation (bit 31 = x^0)
PNG_FN uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(8n) mod P
PNG_FN uint32_t crc_xpow8(uint64_t n) {
    uint32_t r = 0x80000000u, base = 0x00800000u;   // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mulmod(r, base);
        base = crc_mulmod(base, base);
    }
    return r;
}
PNG_FN uint32_t crc_bytes_slow(const uint8_t* p, int n) {   // the few header bytes
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 0xFF) ^ (c >> 8);
    return ~c;
}
PNG_FN void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

// ---- the row filter -----------------------------------------------------------------------------------------------
PNG_FN int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
PNG_FN uint32_t filter_cost(uint8_t v) { return v < 128 ? v : 256u - v; }

struct FilterShared {
    uint32_t total[5];
};

// One row: all five filter types are evaluated, the one with the smallest sum of min(v, 256 - v) is kept (ties: the
// lowest type number), and the row is written as [type][3w filtered bytes].  bpp = 3; the row above row 0 is zeros.
PNG_FN void filter_row(FilterShared& S, const uint8_t* rgb, int32_t w, int32_t row, uint8_t* stream) {
    const int64_t n = (int64_t)w * 3;
    const uint8_t* cur = rgb + (int64_t)row * n;
    const uint8_t* up = row > 0 ? cur - n : nullptr;
    uint8_t* out = stream + (int64_t)row * (n + 1);
    PNG_LANES
        if (t < 5) S.total[t] = 0;
    PNG_SYNC
    PNG_LANES
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
        for (int64_t i = t; i < n; i += kThreads) {
            const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
            s0 += filter_cost((uint8_t)x);
            s1 += filter_cost((uint8_t)(x - a));
            s2 += filter_cost((uint8_t)(x - b));
            s3 += filter_cost((uint8_t)(x - ((a + b) >> 1)));
            s4 += filter_cost((uint8_t)(x - paeth(a, b, c)));
        }
        lds_add(&S.total[0], s0);
        lds_add(&S.total[1], s1);
        lds_add(&S.total[2], s2);
        lds_add(&S.total[3], s3);
        lds_add(&S.total[4], s4);
    PNG_SYNC
    PNG_LANES
        int best = 0;
        for (int k = 1; k < 5; ++k)
            if (S.total[k] < S.total[best]) best = k;
        if (t == 0) out[0] = (uint8_t)best;
        for (int64_t i = t; i < n; i += kThreads) {
            const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
            const int pred = best == 0 ? 0 : best == 1 ? a : best == 2 ? b : best == 3 ? ((a + b) >> 1) : paeth(a, b, c);
            out[1 + i] = (uint8_t)(x - pred);
        }
    PNG_SYNC
}

// ---- one deflate chunk --------------------------------------------------------------------------------------------
struct ChunkShared {
    int32_t head[1 << kHashBits];   // hash of 4 bytes -> 1 + (position - origin) of their latest occurrence; 0 = none
    int32_t head8[1 << kHashBits];  // the same for 8 bytes: the latest place a longer context stood is the likelier long match
    uint32_t lit_freq[288], dist_freq[32], cl_freq[20];
    uint16_t lit_code[288], dist_code[32], cl_code[20];
    uint8_t lit_len[288], dist_len[32], cl_len[20];
    // one tile of 256 positions / symbols
    uint16_t mlen[kThreads], mdist[kThreads];
    uint8_t taken[kThreads], nb[kThreads];
    uint32_t scan[kThreads], scan2[kThreads];
    uint64_t bits[kThreads];
    uint32_t wave_total[kThreads / 64];
    uint32_t stage[kStageWords];
    // Huffman construction
    uint32_t key[288];
    uint32_t sorted_key[288];
    uint16_t sorted_sym[288];
    uint8_t hdr_sym[320], hdr_extra[320];
    // scalars
    int32_t cur, nsym, any_match, n_used, n_hdr, hlit, hdist, hclen;
    uint32_t scan_total, stage_bits, out_pos, carry_byte, use_huffman, est_bytes;
};

// scan[t] -> exclusive prefix sum over the lanes; scan_total = the sum
PNG_FN void block_scan(ChunkShared& S) {
#ifdef ME_PNG_HOST
    uint32_t run = 0;
    for (int t = 0; t < kThreads; ++t) {
        const uint32_t v = S.scan[t];
        S.scan[t] = run;
        run += v;
    }
    S.scan_total = run;
#else
    const int t = (int)threadIdx.x;
    uint32_t all;
    S.scan[t] = me_scan::block_scan<kThreads>(S.scan[t], S.wave_total, all);
    if (t == 0) S.scan_total = all;
    __syncthreads();
#endif
}

PNG_FN uint32_t load32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
PNG_FN uint32_t hash8(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - kHashBits));
}
PNG_FN uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

PNG_FN int match_length(const uint8_t* a, const uint8_t* b, int maxlen) {
    int k = 0;
    while (k + 8 <= maxlen) {
        uint64_t x, y;
        memcpy(&x, a + k, 8);
        memcpy(&y, b + k, 8);
        const uint64_t d = x ^ y;
        if (d) return k + (__builtin_ctzll(d) >> 3);
        k += 8;
    }
    while (k < maxlen && a[k] == b[k]) ++k;
    return k;
}

// RFC 1951 3.2.5: length 3..258 -> code 257..285 + extra bits; distance 1..32768 -> code 0..29 + extra bits
PNG_FN void length_code(int len, int* code, int* nextra, int* extra) {
    const int l = len - 3;
    if (l < 8) { *code = 257 + l, *nextra = 0, *extra = 0; return; }
    if (l == 255) { *code = 285, *nextra = 0, *extra = 0; return; }
    const int nbit = 31 - __builtin_clz((unsigned)l);   // >= 3
    *code = 257 + 4 * (nbit - 1) + ((l >> (nbit - 2)) & 3);
    *nextra = nbit - 2;
    *extra = l & ((1 << (nbit - 2)) - 1);
}
PNG_FN void dist_code(int dist, int* code, int* nextra, int* extra) {
    const int d = dist - 1;
    if (d < 4) { *code = d, *nextra = 0, *extra = 0; return; }
    const int nbit = 31 - __builtin_clz((unsigned)d);   // >= 2
    *code = 2 * nbit + ((d >> (nbit - 1)) & 1);
    *nextra = nbit - 1;
    *extra = d & ((1 << (nbit - 1)) - 1);
}
PNG_FN int length_extra_bits(int code) { return (code < 265 || code == 285) ? 0 : (code - 261) >> 2; }
PNG_FN int dist_extra_bits(int code) { return code < 4 ? 0 : (code >> 1) - 1; }

PNG_FN uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// Lane 0: append n bits (LSB first) to the stage
PNG_FN void stage_put(ChunkShared& S, uint32_t value, int n) {
    const uint32_t pos = S.stage_bits;
    const uint64_t v = (uint64_t)value << (pos & 31);
    S.stage[pos >> 5] |= (uint32_t)v;
    S.stage[(pos >> 5) + 1] |= (uint32_t)(v >> 32);
    S.stage_bits = pos + (uint32_t)n;
}

// The stage's whole bytes go to the slot, its last partial byte is carried to the front.  (Every lane calls it.)
PNG_FN void stage_flush(ChunkShared& S, uint8_t* slot) {
    PNG_LANES
        const uint32_t full = S.stage_bits >> 3;
        for (uint32_t i = t; i < full; i += kThreads) {
            const uint32_t o = S.out_pos + i;
            if (o < (uint32_t)kSlot) slot[o] = (uint8_t)(S.stage[i >> 2] >> ((i & 3) * 8));
        }
    PNG_SYNC
    PNG_LANES
        if (t == 0) {
            const uint32_t full = S.stage_bits >> 3;
            S.carry_byte = (S.stage[full >> 2] >> ((full & 3) * 8)) & 0xFFu;
            S.scan_total = (S.stage_bits + 31) / 32 + 2;   // words to clear
        }
    PNG_SYNC
    PNG_LANES
        const uint32_t words = S.scan_total < (uint32_t)kStageWords ? S.scan_total : (uint32_t)kStageWords;
        for (uint32_t i = t; i < words; i += kThreads) S.stage[i] = i == 0 ? S.carry_byte : 0u;
    PNG_SYNC
    PNG_LANES
        if (t == 0) {
            S.out_pos += S.stage_bits >> 3;
            S.stage_bits &= 7;
        }
    PNG_SYNC
}

// Huffman code lengths of `n` symbols with frequencies freq[], at most max_len bits, and their canonical codes
// (bit-reversed, ready to be written LSB first).  At least two symbols get a code, as zlib does, so that the code is
// complete.  The sort is a rank sort over all lanes; the rest runs on lane 0.
PNG_FN void build_code(ChunkShared& S, const uint32_t* freq, int n, int max_len, uint8_t* len_out, uint16_t* code_out) {
    PNG_LANES
        if (t == 0) {
            int used = 0;
            for (int i = 0; i < n; ++i) {
                S.key[i] = freq[i];
                used += freq[i] != 0;
            }
            if (used < 2 && S.key[0] == 0) S.key[0] = 1, ++used;
            if (used < 2 && S.key[1] == 0) S.key[1] = 1, ++used;
            S.n_used = used;
        }
    PNG_SYNC
    PNG_LANES
        for (int i = t; i < n; i += kThreads) {
            len_out[i] = 0;
            const uint32_t k = S.key[i];
            if (k) {
                int rank = 0;
                for (int j = 0; j < n; ++j) {
                    const uint32_t kj = S.key[j];
                    rank += kj != 0 && (kj < k || (kj == k && j < i));
                }
                S.sorted_key[rank] = k;
                S.sorted_sym[rank] = (uint16_t)i;
            }
        }
    PNG_SYNC
    PNG_LANES
        if (t == 0) {
            uint32_t* A = S.sorted_key;
            const int m = S.n_used;
            // Moffat & Katajainen, in-place calculation of minimum-redundancy code lengths (m >= 2)
            A[0] += A[1];
            int root = 0, leaf = 2, next;
            for (next = 1; next < m - 1; ++next) {
                if (leaf >= m || A[root] < A[leaf]) {
                    A[next] = A[root];
                    A[root++] = (uint32_t)next;
                } else {
                    A[next] = A[leaf++];
                }
                if (leaf >= m || (root < next && A[root] < A[leaf])) {
                    A[next] += A[root];
                    A[root++] = (uint32_t)next;
                } else {
                    A[next] += A[leaf++];
                }
            }
            A[m - 2] = 0;
            for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
            int avbl = 1, used = 0, dpth = 0;
            root = m - 2, next = m - 1;
            while (avbl > 0) {
                while (root >= 0 && (int)A[root] == dpth) ++used, --root;
                while (avbl > used) A[next--] = (uint32_t)dpth, --avbl;
                avbl = 2 * used, ++dpth, used = 0;
            }
            // the number of codes of each length, folded into max_len (miniz's enforce_max_code_size)
            int num[33];
            for (int i = 0; i <= 32; ++i) num[i] = 0;
            for (int i = 0; i < m; ++i) ++num[A[i] > 32 ? 32 : A[i]];
            for (int i = max_len + 1; i <= 32; ++i) num[max_len] += num[i];
            uint32_t total = 0;
            for (int i = max_len; i > 0; --i) total += (uint32_t)num[i] << (max_len - i);
            while (total != (1u << max_len)) {
                --num[max_len];
                for (int i = max_len - 1; i > 0; --i)
                    if (num[i]) {
                        --num[i];
                        num[i + 1] += 2;
                        break;
                    }
                --total;
            }
            // the most frequent symbols (the end of the ascending order) get the shortest codes
            int j = m;
            for (int i = 1; i <= max_len; ++i)
                for (int l = num[i]; l > 0; --l) len_out[S.sorted_sym[--j]] = (uint8_t)i;
            uint32_t next_code[17];
            next_code[0] = next_code[1] = 0;
            for (int i = 2; i <= max_len; ++i) next_code[i] = (next_code[i - 1] + (uint32_t)num[i - 1]) << 1;
            for (int i = 0; i < n; ++i) {
                const int l = len_out[i];
                code_out[i] = l ? (uint16_t)reverse_bits(next_code[l]++, l) : (uint16_t)0;
            }
        }
    PNG_SYNC
}

// Chunk c of the filtered stream in[0, total) -> its deflate bytes in slot[0, kSlot), the parsed symbols in
// syms[0, kChunk) on the way (literal: the byte; match: bit 31 | (len - 3) << 15 | (dist - 1)).
PNG_FN void deflate_chunk(ChunkShared& S, const uint8_t* in, int64_t total, int64_t stride, int64_t c, int64_t nchunks,
                          uint32_t* syms, uint8_t* slot, ChunkInfo* info) {
    const int64_t base = c * kChunk;
    const int32_t N = (int32_t)(total - base < kChunk ? total - base : kChunk);
    const int32_t P = (int32_t)(base < kWindow ? base : kWindow);   // a multiple of 256
    const int64_t origin = base - P;
    const bool last = c == nchunks - 1;
    const uint8_t* src = in + base;

    PNG_LANES
        for (int i = t; i < (1 << kHashBits); i += kThreads) S.head[i] = 0, S.head8[i] = 0;
        for (int i = t; i < 288; i += kThreads) S.lit_freq[i] = 0;
        if (t < 32) S.dist_freq[t] = 0;
        if (t < 20) S.cl_freq[t] = 0;
        for (int i = t; i < kStageWords; i += kThreads) S.stage[i] = 0;
        if (t == 0) S.cur = 0, S.nsym = 0, S.stage_bits = 0, S.out_pos = 0;
        // Adler-32 partial sums of the chunk
        uint64_t a = 0, b = 0;
        for (int32_t i = t; i < N; i += kThreads) {
            const uint32_t d = src[i];
            a += d;
            b += (uint64_t)(N - i) * d;
        }
        S.scan[t] = (uint32_t)(a % 65521u);
        S.scan2[t] = (uint32_t)(b % 65521u);
    PNG_SYNC
    PNG_LANES
        if (t == 0) {
            uint32_t a = 0, b = 0;
            for (int i = 0; i < kThreads; ++i) a += S.scan[i], b += S.scan2[i];   // < 2^24 each
            info->adler_a = a % 65521u;
            info->adler_b = b % 65521u;
        }
    PNG_SYNC

    // ---- LZ77: tiles of 256 positions in order; a tile looks its candidates up, then inserts itself -----------------
    for (int32_t tile = -P; tile < N; tile += kThreads) {
        PNG_LANES
            const int32_t q = tile + t;
            const int64_t g = base + q;
            int ml = 0, md = 0;
            if (t == 0) S.any_match = 0;
            if (q >= 0 && q < N && g + 3 < total) {
                const int32_t cand = S.head[hash4(load32(in + g))];
                const int maxlen = N - q < kMaxMatch ? N - q : kMaxMatch;
                if (maxlen >= kMinMatch) {
                    // the candidates: the latest earlier occurrence of these 4 and of these 8 bytes, and the fixed distances
                    // at which a filtered picture repeats (the byte, the pixel and the row before); the longest wins,
                    // then the nearest
                    const int32_t cand8 = g + 7 < total ? S.head8[hash8(in + g)] : 0;
                    const int64_t dists[5] = {cand > 0 ? g - (origin + (cand - 1)) : 0,
                                              cand8 > 0 ? g - (origin + (cand8 - 1)) : 0, 1, 3, stride};
                    for (int k = 0; k < 5; ++k) {
                        const int64_t dist = dists[k];
                        if (dist < 1 || dist > kMaxDist || dist > g) continue;
                        const int l = match_length(in + g - dist, in + g, maxlen);
                        if (l >= kMinMatch && (l > ml || (l == ml && dist < md))) ml = l, md = (int)dist;
                    }
                }
            }
            S.mlen[t] = (uint16_t)ml;
            S.mdist[t] = (uint16_t)(md - 1);
            S.taken[t] = 0;
        PNG_SYNC
        PNG_LANES
            const int64_t g = base + tile + t;
            if (tile + t < N && g + 3 < total) lds_max(&S.head[hash4(load32(in + g))], (int32_t)(g - origin) + 1);
            if (tile + t < N && g + 7 < total) lds_max(&S.head8[hash8(in + g)], (int32_t)(g - origin) + 1);
            if (S.mlen[t]) S.any_match = 1;
        PNG_SYNC
        if (tile < 0) continue;
        // the greedy parse: which positions start a symbol
        PNG_LANES
            if (S.any_match) {
                if (t == 0) {
                    int32_t p = S.cur;
                    const int32_t end = tile + kThreads < N ? tile + kThreads : N;
                    while (p < end) {
                        S.taken[p - tile] = 1;
                        int l = S.mlen[p - tile];
                        // lazy: a longer match one byte on makes this byte a literal
                        if (l && l < kLazyBelow && p + 1 < end && S.mlen[p + 1 - tile] > l) S.mlen[p - tile] = 0, l = 0;
                        p += l ? l : 1;
                    }
                    S.cur = p;
                }
            } else {
                S.taken[t] = (tile + t >= S.cur && tile + t < N) ? 1 : 0;
            }
        PNG_SYNC
        PNG_LANES
            if (t == 0 && !S.any_match) {
                const int32_t end = tile + kThreads < N ? tile + kThreads : N;
                if (S.cur < end) S.cur = end;
            }
            S.scan[t] = S.taken[t];
        PNG_SYNC
        block_scan(S);
        PNG_LANES
            if (S.taken[t]) {
                const int32_t q = tile + t;
                const uint32_t idx = (uint32_t)S.nsym + S.scan[t];
                const int l = S.mlen[t];
                if (l) {
                    const int d = (int)S.mdist[t] + 1;
                    int code, nx, ex;
                    length_code(l, &code, &nx, &ex);
                    lds_add(&S.lit_freq[code], 1u);
                    dist_code(d, &code, &nx, &ex);
                    lds_add(&S.dist_freq[code], 1u);
                    syms[idx] = 0x80000000u | ((uint32_t)(l - 3) << 15) | (uint32_t)(d - 1);
                } else {
                    const uint32_t v = src[q];
                    lds_add(&S.lit_freq[v], 1u);
                    syms[idx] = v;
                }
            }
        PNG_SYNC
        PNG_LANES
            if (t == 0) S.nsym += (int32_t)S.scan_total;
        PNG_SYNC
    }

    // ---- the dynamic Huffman block's codes and header ---------------------------------------------------------------
    PNG_LANES
        if (t == 0) S.lit_freq[256] = 1;
    PNG_SYNC
    build_code(S, S.lit_freq, 286, 15, S.lit_len, S.lit_code);
    build_code(S, S.dist_freq, 30, 15, S.dist_len, S.dist_code);
    PNG_LANES
        if (t == 0) {
            int hlit = 286, hdist = 30;
            while (hlit > 257 && S.lit_len[hlit - 1] == 0) --hlit;
            while (hdist > 1 && S.dist_len[hdist - 1] == 0) --hdist;
            S.hlit = hlit, S.hdist = hdist;
            // RFC 1951 3.2.7: the lengths of both codes as one sequence, run-length coded with 16 / 17 / 18
            const int all = hlit + hdist;
            int nh = 0, i = 0;
            while (i < all) {
                const int v = i < hlit ? S.lit_len[i] : S.dist_len[i - hlit];
                int run = 1;
                while (i + run < all && (i + run < hlit ? S.lit_len[i + run] : S.dist_len[i + run - hlit]) == v) ++run;
                i += run;
                if (v == 0) {
                    while (run >= 11) {
                        const int r = run < 138 ? run : 138;
                        S.hdr_sym[nh] = 18, S.hdr_extra[nh++] = (uint8_t)(r - 11);
                        run -= r;
                    }
                    if (run >= 3) {
                        S.hdr_sym[nh] = 17, S.hdr_extra[nh++] = (uint8_t)(run - 3);
                        run = 0;
                    }
                    while (run-- > 0) S.hdr_sym[nh] = 0, S.hdr_extra[nh++] = 0;
                } else {
                    S.hdr_sym[nh] = (uint8_t)v, S.hdr_extra[nh++] = 0;
                    --run;
                    while (run >= 3) {
                        const int r = run < 6 ? run : 6;
                        S.hdr_sym[nh] = 16, S.hdr_extra[nh++] = (uint8_t)(r - 3);
                        run -= r;
                    }
                    while (run-- > 0) S.hdr_sym[nh] = (uint8_t)v, S.hdr_extra[nh++] = 0;
                }
            }
            S.n_hdr = nh;
            for (int k = 0; k < nh; ++k) ++S.cl_freq[S.hdr_sym[k]];
        }
    PNG_SYNC
    build_code(S, S.cl_freq, 19, 7, S.cl_len, S.cl_code);
    PNG_LANES
        if (t == 0) {
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            int hclen = 19;
            while (hclen > 4 && S.cl_len[order[hclen - 1]] == 0) --hclen;
            S.hclen = hclen;
            // the exact size of the block, against the chunk stored
            uint64_t bits = 3 + 14 + 3 * (uint64_t)hclen;
            for (int k = 0; k < S.n_hdr; ++k) {
                const int s = S.hdr_sym[k];
                bits += S.cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
            }
            for (int s = 0; s < 286; ++s) bits += (uint64_t)S.lit_freq[s] * (S.lit_len[s] + (s > 256 ? length_extra_bits(s) : 0));
            for (int s = 0; s < 30; ++s) bits += (uint64_t)S.dist_freq[s] * (S.dist_len[s] + dist_extra_bits(s));
            if (!last) bits += 3;
            const uint64_t huff_bytes = (bits + 7) / 8 + (last ? 0 : 4);
            const uint32_t nblocks = ((uint32_t)N + 65534u) / 65535u;
            const uint64_t stored_bytes = (uint64_t)N + 5ull * nblocks;
            S.use_huffman = huff_bytes <= stored_bytes;
            S.est_bytes = (uint32_t)(S.use_huffman ? huff_bytes : stored_bytes);
            if (S.use_huffman) {
                stage_put(S, last ? 1u : 0u, 1);
                stage_put(S, 2u, 2);
                stage_put(S, (uint32_t)(S.hlit - 257), 5);
                stage_put(S, (uint32_t)(S.hdist - 1), 5);
                stage_put(S, (uint32_t)(hclen - 4), 4);
                for (int k = 0; k < hclen; ++k) stage_put(S, S.cl_len[order[k]], 3);
                for (int k = 0; k < S.n_hdr; ++k) {
                    const int s = S.hdr_sym[k];
                    stage_put(S, S.cl_code[s], S.cl_len[s]);
                    if (s >= 16) stage_put(S, S.hdr_extra[k], s == 16 ? 2 : s == 17 ? 3 : 7);
                }
            }
        }
    PNG_SYNC

    if (!S.use_huffman) {
        // stored blocks: BFINAL/BTYPE byte, LEN, NLEN, the bytes
        PNG_LANES
            const int32_t nblocks = (N + 65534) / 65535;
            if (t < nblocks) {
                const int32_t off = t * 65535, len = N - off < 65535 ? N - off : 65535;
                uint8_t* h = slot + (int64_t)off + 5 * t;
                h[0] = (last && t == nblocks - 1) ? 1 : 0;
                h[1] = (uint8_t)len, h[2] = (uint8_t)(len >> 8);
                h[3] = (uint8_t)~len, h[4] = (uint8_t)(~len >> 8);
            }
            for (int32_t i = t; i < N; i += kThreads) slot[i + 5 * (i / 65535 + 1)] = src[i];
            if (t == 0) {
                info->nbytes = S.est_bytes;
                info->flags = 1;
            }
        PNG_SYNC
        return;
    }

    stage_flush(S, slot);
    // ---- bit packing: 256 symbols at a time, each at the prefix sum of the bit counts before it ---------------------
    for (int32_t s0 = 0; s0 < S.nsym; s0 += kThreads) {
        PNG_LANES
            uint64_t v = 0;
            int n = 0;
            if (s0 + t < S.nsym) {
                const uint32_t w = syms[s0 + t];
                if (w & 0x80000000u) {
                    int code, nx, ex;
                    length_code((int)((w >> 15) & 0xFF) + 3, &code, &nx, &ex);
                    v = S.lit_code[code], n = S.lit_len[code];
                    v |= (uint64_t)ex << n, n += nx;
                    dist_code((int)(w & 0x7FFF) + 1, &code, &nx, &ex);
                    v |= (uint64_t)S.dist_code[code] << n, n += S.dist_len[code];
                    v |= (uint64_t)ex << n, n += nx;
                } else {
                    v = S.lit_code[w], n = S.lit_len[w];
                }
            }
            S.bits[t] = v;
            S.nb[t] = (uint8_t)n;
            S.scan[t] = (uint32_t)n;
        PNG_SYNC
        block_scan(S);
        PNG_LANES
            if (S.nb[t]) {
                const uint32_t pos = S.stage_bits + S.scan[t];
                const uint32_t sh = pos & 31, wi = pos >> 5;
                const uint64_t v = S.bits[t];
                lds_or(&S.stage[wi], (uint32_t)(v << sh));
                const uint64_t hi = sh ? (v >> (32 - sh)) : (v >> 32);
                if ((uint32_t)hi) lds_or(&S.stage[wi + 1], (uint32_t)hi);
                if ((uint32_t)(hi >> 32)) lds_or(&S.stage[wi + 2], (uint32_t)(hi >> 32));
            }
        PNG_SYNC
        PNG_LANES
            if (t == 0) S.stage_bits += S.scan_total;
        PNG_SYNC
        stage_flush(S, slot);
    }
    PNG_LANES
        if (t == 0) {
            stage_put(S, S.lit_code[256], S.lit_len[256]);
            if (!last) stage_put(S, 0u, 3);                   // an empty stored block: BFINAL 0, BTYPE 00
            S.stage_bits = (S.stage_bits + 7) & ~7u;          // to the byte boundary
            if (!last) {
                stage_put(S, 0x0000u, 16);                    // LEN 0
                stage_put(S, 0xFFFFu, 16);                    // NLEN
            }
        }
    PNG_SYNC
    stage_flush(S, slot);
    PNG_LANES
        if (t == 0) {
            info->nbytes = S.out_pos < (uint32_t)kSlot ? S.out_pos : (uint32_t)kSlot;
            info->flags = S.out_pos != S.est_bytes ? 2u : 0u;
        }
    PNG_SYNC
}

// ---- the file -----------------------------------------------------------------------------------------------------
// Lane 0 of one workgroup: where every IDAT starts, the stream's Adler-32, the file's size, and the fixed bytes.
// meta[0] = size of the file, meta[1] = Adler-32, meta[2] = OR of the chunks' flags.
PNG_FN void layout_file(const ChunkInfo* info, int64_t nchunks, int32_t w, int32_t h, uint8_t* file, int64_t* offsets,
                        int64_t* meta) {
    PNG_LANES
        if (t == 0) {
            const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
            for (int i = 0; i < 8; ++i) file[i] = sig[i];
            uint8_t* p = file + 8;
            put_be32(p, 13);
            p[4] = 'I', p[5] = 'H', p[6] = 'D', p[7] = 'R';
            put_be32(p + 8, (uint32_t)w);
            put_be32(p + 12, (uint32_t)h);
            p[16] = 8, p[17] = 2, p[18] = 0, p[19] = 0, p[20] = 0;   // 8 bits, RGB, deflate, adaptive filters, no interlace
            put_be32(p + 21, crc_bytes_slow(p + 4, 17));
            int64_t pos = kFileHead;
            uint32_t a = 1, b = 0, flags = 0;
            for (int64_t c = 0; c < nchunks; ++c) {
                offsets[c] = pos;
                const uint32_t n = info[c].nbytes;
                pos += 12 + (int64_t)n + (c == 0 ? 2 : 0) + (c == nchunks - 1 ? 4 : 0);
                const uint32_t len = (uint32_t)(c == nchunks - 1 ? ((int64_t)w * 3 + 1) * h - c * kChunk : kChunk);
                b = (uint32_t)((b + (uint64_t)(len % 65521u) * a + info[c].adler_b) % 65521u);
                a = (a + info[c].adler_a) % 65521u;
                flags |= info[c].flags;
            }
            const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
            for (int i = 0; i < 12; ++i) file[pos + i] = iend[i];
            meta[0] = pos + 12;
            meta[1] = ((int64_t)b << 16) | a;
            meta[2] = flags;
        }
    PNG_SYNC
}

struct GatherShared {
    uint32_t table[256];
    uint32_t part[kThreads];
};

// IDAT c: length, "IDAT", [zlib header] the chunk's deflate bytes [Adler-32], CRC-32.  The CRC: every lane takes an
// equal slice of (leading zero padding +) type + data from a zero register, and the slices are combined by
// crc(A || B) = crc(A) * x^(8 |B|) + crc(B); the 0xFFFFFFFF the register starts from is added the same way.
PNG_FN void gather_idat(GatherShared& S, const ChunkInfo* info, const uint8_t* slot, int64_t c, int64_t nchunks,
                        const int64_t* offsets, const int64_t* meta, uint8_t* file) {
    const uint32_t n = info[c].nbytes;
    const uint32_t pre = c == 0 ? 2u : 0u, post = c == nchunks - 1 ? 4u : 0u;
    const uint32_t data = pre + n + post;
    const uint32_t L = 4 + data;                  // what the CRC covers
    uint8_t* out = file + offsets[c];
    uint8_t* body = out + 8 + pre;
    PNG_LANES
        S.table[t] = crc_table_entry((uint32_t)t);
        if (t == 0) {
            put_be32(out, data);
            out[4] = 'I', out[5] = 'D', out[6] = 'A', out[7] = 'T';
            if (pre) out[8] = 0x78, out[9] = 0xDA;   // deflate, 32 KiB window; FLEVEL 3; (0x78DA % 31 == 0)
            if (post) put_be32(body + n, (uint32_t)meta[1]);
        }
        for (uint32_t i = t; i < n; i += kThreads) body[i] = slot[i];
    PNG_SYNC
    const uint32_t per = (L + kThreads - 1) / kThreads, pad = per * kThreads - L;
    PNG_LANES
        uint32_t r = 0;
        const uint8_t* p = out + 4;               // the type; this workgroup wrote every byte of [p, p + L)
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t v = (uint32_t)t * per + k;
            if (v >= pad) r = S.table[(r ^ p[v - pad]) & 0xFF] ^ (r >> 8);
        }
        S.part[t] = r;
    PNG_SYNC
    PNG_LANES
        if (t == 0) {
            const uint32_t X = crc_xpow8(per);
            uint32_t s = 0;
            for (int k = 0; k < kThreads; ++k) s = crc_mulmod(s, X) ^ S.part[k];
            s ^= crc_mulmod(0xFFFFFFFFu, crc_xpow8(L));
            put_be32(body + n + post, ~s);
        }
    PNG_SYNC
}

}  // namespace me_png
