// Huffman decoding of a sequential JPEG scan by one thread per SUBSEQUENCE of S bits, integer for integer the coefficients of
// host/jpeg_decoder.cpp (Decoder::decode_scan / block_sequential).  A Huffman decoder started at a wrong bit falls into step
// with the right one after a while; that makes the scan decodable in parallel with an exact result:
//
//   speculate   thread i decodes the symbols that start inside subsequence i from a cold state (bit i * S, block 0 of the
//               MCU, a DC symbol next) and records its end state (bit, block in MCU, zigzag index)
//   sync        rounds: every thread whose predecessor's end state changed in the round before decodes its subsequence again
//               from that state.  Subsequence 0 of a segment starts from the true state, so the fixed point IS the sequential
//               decode; a round without a change confirms it.  Round r makes the end state that a cold start r subsequences
//               back gives (Jacobi: three rotating buffers, no thread reads what another writes in the same round)
//   scan        per segment, exclusive sums of the blocks completed and of the DC differences per component: each thread's
//               first block ordinal and DC predictors (the .hip file on the device, a loop in the host driver)
//   write       thread i decodes its subsequence from its true start state and stores the coefficients
//
// A cold start can meet an invalid code or an AC run past 63; both are normal there (16 bits consumed / the block ended) and
// count as errors only in the write pass, which runs the true chain.  Every loop consumes at least one bit per turn and ends
// with the bits of its subsequence.
//
// The per-thread routines are plain functions of (tables, stream, thread index): the bodies of the kernels of
// csrc/jpeg_entropy.hip and, with ME_JPEG_HOST defined, plain C++ that tests/jpeg_entropy_host.cpp runs thread by thread.
// The host half (prepare) destuffs the scan and lays out what is uploaded; it is the same code in both builds.
#pragma once
#ifndef ME_JPEG_HOST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../host/image_io.hpp"

namespace me_jpeg_entropy {

#ifdef ME_JPEG_HOST
#define JE_FN inline
#else
#define JE_FN __device__ inline
#endif

constexpr int kThreads = 256;               // subsequences of one workgroup
constexpr int kMinSubseqBits = 64;          // a symbol is at most 31 bits
constexpr int kDefaultSubseqBits = 1024;
constexpr int kMaxSubseqBits = 65536;
constexpr int kGiveUpBits = 65536;          // sync distance after which the decoder declines (8x the worst seen)
constexpr int kMaxMcuBlocks = 10;           // T.81 B.2.3
constexpr int kRoundsPerBatch = 8;          // sync rounds queued between two looks at the changed counts

// Canonical Huffman table for a left-aligned 16-bit window `c`: the code's length is 1 + the number of l in 1..16 with
// c >= limit[l] (limit[l] = first code behind those of length <= l, left-aligned: non-decreasing for a prefix code), its value
// values[delta[l] + (c >> (16 - l))].  lut answers codes of up to 8 bits in one read: length << 8 | value, 0 = longer.
struct HuffDev {
    uint16_t lut[256];
    uint32_t limit[17];
    int32_t delta[17];
    uint8_t values[256];
};
struct ScanDesc {
    int32_t nb;                      // blocks per MCU
    int32_t mcus_x, total_mcus;
    int32_t interval;                // MCUs per segment (the restart interval, or all of them)
    int32_t nseg, nsub, subseq_bits;
    uint8_t blk_comp[kMaxMcuBlocks], blk_x[kMaxMcuBlocks], blk_y[kMaxMcuBlocks];   // block b of the MCU: frame component, place
    uint8_t blk_dc[kMaxMcuBlocks], blk_ac[kMaxMcuBlocks];                         // ... and its tables (ac: 4 + selector)
    int32_t comp_h[3], comp_v[3], comp_blocks_w[3];
    int64_t comp_coef_off[3];        // int16_t index of the component's first coefficient (jpeg_idct_kernel's layout)
};
struct EntropyTables {
    HuffDev huff[8];                 // 0..3 DC, 4..7 AC
    ScanDesc scan;
};
static_assert(sizeof(EntropyTables) % 8 == 0, "staged as dwords, holds int64_t");

// what a subsequence's decode leaves behind besides its end state
struct alignas(16) Counts {
    int32_t blocks;                  // blocks completed
    uint32_t dc[3];                  // sum of the DC differences per frame component, modulo 2^32 like the host's int
};

// decoder state between two symbols: bit position in the destuffed stream, block inside the MCU, zigzag index (0: DC next)
JE_FN uint64_t pack_state(uint32_t pos, int b, int k) { return ((uint64_t)pos << 32) | ((uint32_t)b << 8) | (uint32_t)k; }
JE_FN uint32_t state_pos(uint64_t s) { return (uint32_t)(s >> 32); }
JE_FN int state_b(uint64_t s) { return (int)((s >> 8) & 0xff); }
JE_FN int state_k(uint64_t s) { return (int)(s & 0xff); }

constexpr uint8_t kZigzagNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// 32 bits of the stream from bit `pos`, big-endian as the file has them; bits at and behind `end` (the segment's) read as
// zeros (BitReader::fill, T.81 F.2.2.5).  `words` holds two dwords more than the stream.
JE_FN uint32_t peek32(const uint32_t* words, uint32_t pos, uint32_t end) {
    if (pos >= end) return 0;
    const uint32_t d = pos >> 5;
    const uint64_t v = ((uint64_t)__builtin_bswap32(words[d]) << 32) | __builtin_bswap32(words[d + 1]);
    uint32_t w = (uint32_t)((v << (pos & 31)) >> 32);
    const uint32_t left = end - pos;
    if (left < 32) w &= ~0u << (32 - left);
    return w;
}

// what the write pass carries along
struct WriteState {
    int16_t* coef;
    int32_t blk, blk_end;            // ordinal of the block in progress within the scan; the segment's last + 1
    uint32_t pred[3];
    int64_t base;                    // coefficient index of the block in progress
    int32_t error;                   // JpegEntropyDecline of the true chain, 0: none
};

JE_FN int64_t block_base(const ScanDesc& sc, int32_t blk, int b) {
    const int32_t m = blk / sc.nb, uy = m / sc.mcus_x, ux = m - uy * sc.mcus_x;
    const int c = sc.blk_comp[b];
    const int32_t bx = ux * sc.comp_h[c] + sc.blk_x[b], by = uy * sc.comp_v[c] + sc.blk_y[b];
    return sc.comp_coef_off[c] + ((int64_t)by * sc.comp_blocks_w[c] + bx) * 64;
}

// Decodes the symbols that start in [pos of `state`, sub_end) of one segment; one body for all passes, the table chosen by
// k == 0 as an index.  kWrite: the true chain -- coefficients are stored, and garbage is an error.
template <bool kWrite>
JE_FN uint64_t decode_range(const EntropyTables& t, const uint32_t* words, uint64_t state, uint32_t sub_end, uint32_t seg_end,
                            Counts& cnt, WriteState* w) {
    const ScanDesc& sc = t.scan;
    uint32_t pos = state_pos(state);
    int b = state_b(state), k = state_k(state);
    cnt.blocks = 0, cnt.dc[0] = cnt.dc[1] = cnt.dc[2] = 0;
    while (pos < sub_end && (!kWrite || w->blk < w->blk_end)) {
        const uint32_t win = peek32(words, pos, seg_end);
        const HuffDev& h = t.huff[k == 0 ? sc.blk_dc[b] : sc.blk_ac[b]];
        const uint32_t c16 = win >> 16;
        const uint32_t e = h.lut[win >> 24];
        int len = (int)(e >> 8), value = (int)(e & 255);
        if (len == 0) {
            len = 1;
            for (int l = 1; l <= 16; ++l) len += c16 >= h.limit[l] ? 1 : 0;
            if (len > 16) {  // no such code: 16 bits are gone, the state stays
                pos += 16;
                if (kWrite) w->error = matrix_eyes::kJpegDeclineBadCode;
                continue;
            }
            value = h.values[(h.delta[len] + (int32_t)(c16 >> (16 - len))) & 255];
        }
        const int s = value & 15, r = k == 0 ? 0 : value >> 4;
        // receive_extend: s bits behind the code
        int32_t v = s ? (int32_t)((win << len) >> (32 - s)) : 0;
        if (s && v < (1 << (s - 1))) v -= (1 << s) - 1;
        pos += (uint32_t)(len + s);
        bool done = false;
        if (k == 0) {
            const int c = sc.blk_comp[b];  // selects, not an index: the sums stay in registers
            cnt.dc[0] += c == 0 ? (uint32_t)v : 0u, cnt.dc[1] += c == 1 ? (uint32_t)v : 0u, cnt.dc[2] += c == 2 ? (uint32_t)v : 0u;
            if (kWrite) {
                w->pred[0] += c == 0 ? (uint32_t)v : 0u, w->pred[1] += c == 1 ? (uint32_t)v : 0u, w->pred[2] += c == 2 ? (uint32_t)v : 0u;
                w->coef[w->base] = (int16_t)(c == 0 ? w->pred[0] : (c == 1 ? w->pred[1] : w->pred[2]));
            }
            k = 1;
        } else if (s == 0) {
            if (r == 15) {
                k += 16;
                done = k > 63;
            } else {
                done = true;
            }
        } else {
            k += r;
            if (k > 63) {  // a run past the block: it ends here
                done = true;
                if (kWrite) w->error = matrix_eyes::kJpegDeclineBadRun;
            } else {
                if (kWrite) w->coef[w->base + kZigzagNatural[k]] = (int16_t)v;
                done = ++k > 63;
            }
        }
        if (done) {
            k = 0;
            b = b + 1 == sc.nb ? 0 : b + 1;
            ++cnt.blocks;
            if (kWrite) {
                ++w->blk;
                if (w->blk < w->blk_end) w->base = block_base(sc, w->blk, b);
            }
        }
    }
    return pack_state(pos, b, k);
}

// ---- what every pass reads: the stream and the tables of its segments and subsequences ----------------------------------
struct Stream {
    const EntropyTables* tables;
    const uint32_t* words;           // the destuffed scan; segment j starts on a dword
    const uint32_t* seg_bit0;        // first bit of segment j
    const uint32_t* seg_bits;        // its length
    const int32_t* seg_sub0;         // its first subsequence
    const int32_t* sub_seg;          // segment of subsequence i
};
struct SubRange {
    int32_t seg;
    bool head, tail;                 // first / last subsequence of its segment
    uint32_t begin, end, seg_end;
};
JE_FN SubRange sub_range(const Stream& st, const ScanDesc& sc, int32_t i) {
    SubRange r;
    r.seg = st.sub_seg[i];
    const int32_t local = i - st.seg_sub0[r.seg];
    r.head = local == 0;
    r.tail = i + 1 == sc.nsub || st.sub_seg[i + 1] != r.seg;
    r.seg_end = st.seg_bit0[r.seg] + st.seg_bits[r.seg];
    r.begin = st.seg_bit0[r.seg] + (uint32_t)local * (uint32_t)sc.subseq_bits;
    if (r.begin > r.seg_end) r.begin = r.seg_end;
    r.end = r.tail ? r.seg_end : r.begin + (uint32_t)sc.subseq_bits;
    return r;
}

// speculate: thread i
JE_FN void speculate_thread(const EntropyTables& t, const Stream& st, int32_t i, uint64_t* state0, Counts* counts) {
    const SubRange r = sub_range(st, t.scan, i);
    Counts c;
    state0[i] = decode_range<false>(t, st.words, pack_state(r.begin, 0, 0), r.end, r.seg_end, c, nullptr);
    counts[i] = c;
}

// sync round: thread i.  in / prev: the end states of the round before and of the one before that (prev == nullptr in the
// first round: everybody decodes).  Returns 1 when the thread's end state changed.
JE_FN int sync_thread(const EntropyTables& t, const Stream& st, int32_t i, const uint64_t* prev, const uint64_t* in, uint64_t* out,
                      Counts* counts) {
    const SubRange r = sub_range(st, t.scan, i);
    const uint64_t mine = in[i];
    if (r.head || (prev && prev[i - 1] == in[i - 1])) {
        out[i] = mine;
        return 0;
    }
    Counts c;
    const uint64_t now = decode_range<false>(t, st.words, in[i - 1], r.end, r.seg_end, c, nullptr);
    out[i] = now;
    counts[i] = c;
    return now != mine ? 1 : 0;
}

// write: thread i, from its true start state (the cold one at a segment's head, else its predecessor's end state) and the
// exclusive sums of `counts` over its segment.  Returns the JpegEntropyDecline of the true chain, 0: none.
JE_FN int write_thread(const EntropyTables& t, const Stream& st, int32_t i, const uint64_t* final_state, const Counts* before,
                       int16_t* coef) {
    const ScanDesc& sc = t.scan;
    const SubRange r = sub_range(st, sc, i);
    const uint64_t start = r.head ? pack_state(r.begin, 0, 0) : final_state[i - 1];
    const int32_t seg_blk0 = r.seg * sc.interval * sc.nb;
    int32_t seg_mcus = sc.total_mcus - r.seg * sc.interval;
    if (seg_mcus > sc.interval) seg_mcus = sc.interval;
    WriteState w;
    w.coef = coef, w.error = 0;
    w.blk = seg_blk0 + before[i].blocks, w.blk_end = seg_blk0 + seg_mcus * sc.nb;
    w.pred[0] = before[i].dc[0], w.pred[1] = before[i].dc[1], w.pred[2] = before[i].dc[2];
    w.base = w.blk < w.blk_end ? block_base(sc, w.blk, state_b(start)) : 0;
    Counts c;
    decode_range<true>(t, st.words, start, r.end, r.seg_end, c, &w);
    if (!w.error && r.tail && w.blk < w.blk_end) w.error = matrix_eyes::kJpegDeclineShort;
    return w.error;
}

// ---- the host half ----------------------------------------------------------------------------------------------------------
inline void build_huffman(const matrix_eyes::JpegHuffmanSpec& s, HuffDev& h) {
    memset(&h, 0, sizeof(h));
    memcpy(h.values, s.values, 256);
    uint32_t code = 0;   // next code of the current length
    int k = 0;           // its index into values
    for (int len = 1; len <= 16; ++len) {
        h.delta[len] = k - (int32_t)code;
        const int n = s.counts[len - 1];
        if (len <= 8)
            for (int j = 0; j < n; ++j)
                for (uint32_t fill = 0; fill < (1u << (8 - len)); ++fill) {
                    const uint32_t at = ((code + (uint32_t)j) << (8 - len)) | fill;
                    if (at < 256) h.lut[at] = (uint16_t)(len << 8 | s.values[(k + j) & 255]);
                }
        code += (uint32_t)n, k += n;
        h.limit[len] = code << (16 - len);
        code <<= 1;
    }
}

inline int32_t rounds_allowed(int32_t subseq_bits) { return (kGiveUpBits + subseq_bits - 1) / subseq_bits + 1; }

// where the parts of one upload lie, in dwords from its start
struct Layout {
    size_t words = 0, seg_bit0 = 0, seg_bits = 0, seg_sub0 = 0, sub_seg = 0, total = 0;
    int32_t nseg = 0, nsub = 0;
};
// an upper bound of Layout::total for an eligible plan: the destuffed stream is no longer than the scan
inline size_t upload_capacity(const matrix_eyes::JpegEntropyPlan& p, int32_t subseq_bits) {
    const size_t nseg = p.seg_begin.size(), bytes = p.scan_end - p.scan_begin;
    const size_t stream = bytes / 4 + nseg + 4, nsub = bytes * 8 / (size_t)subseq_bits + nseg;
    return sizeof(EntropyTables) / 4 + stream + 3 * nseg + nsub;
}
// Fills `buf` (upload_capacity dwords) with the tables, the destuffed stream and the segment / subsequence tables of an
// eligible plan: one pass over the scan's bytes, from 0xFF to 0xFF.
inline Layout prepare(const matrix_eyes::JpegEntropyPlan& p, const uint8_t* file, int32_t subseq_bits, uint32_t* buf) {
    Layout lay;
    EntropyTables& t = *reinterpret_cast<EntropyTables*>(buf);
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < 4; ++i) {
        if (p.dc[i].present) build_huffman(p.dc[i], t.huff[i]);
        if (p.ac[i].present) build_huffman(p.ac[i], t.huff[4 + i]);
    }
    ScanDesc& sc = t.scan;
    int64_t coef_off[3] = {0, 0, 0}, off = 0;
    for (size_t c = 0; c < p.frame.comps.size() && c < 3; ++c) {
        coef_off[c] = off;
        off += (int64_t)p.frame.comps[c].blocks_w * p.frame.comps[c].blocks_h * 64;
    }
    for (int i = 0; i < p.scan_comps; ++i) {
        const int c = p.scan_comp[i];
        const matrix_eyes::JpegComponent& k = p.frame.comps[(size_t)c];
        sc.comp_h[c] = k.h, sc.comp_v[c] = k.v, sc.comp_blocks_w[c] = k.blocks_w, sc.comp_coef_off[c] = coef_off[c];
        for (int y = 0; y < k.v; ++y)
            for (int x = 0; x < k.h; ++x) {
                const int b = sc.nb++;
                sc.blk_comp[b] = (uint8_t)c, sc.blk_x[b] = (uint8_t)x, sc.blk_y[b] = (uint8_t)y;
                sc.blk_dc[b] = (uint8_t)p.scan_td[i], sc.blk_ac[b] = (uint8_t)(4 + p.scan_ta[i]);
            }
    }
    sc.mcus_x = p.mcus_x, sc.total_mcus = p.mcus_x * p.mcus_y;
    sc.interval = p.restart_interval ? p.restart_interval : sc.total_mcus;
    sc.subseq_bits = subseq_bits;
    const size_t nseg = p.seg_begin.size();
    sc.nseg = lay.nseg = (int32_t)nseg;
    lay.words = sizeof(EntropyTables) / 4;  // the tables come first
    // the stream: each segment from a dword boundary, FF 00 -> FF
    uint8_t* out = reinterpret_cast<uint8_t*>(buf + lay.words);
    std::vector<uint32_t> bit0(nseg), bits(nseg);
    size_t at = 0;
    for (size_t j = 0; j < nseg; ++j) {
        while (at & 3) out[at++] = 0;
        bit0[j] = (uint32_t)(at * 8);
        const uint8_t* s = file + p.seg_begin[j];
        const uint8_t* e = file + p.seg_end[j];
        while (s < e) {
            const uint8_t* ff = (const uint8_t*)memchr(s, 0xff, (size_t)(e - s));
            const size_t n = (size_t)((ff ? ff + 1 : e) - s);
            memcpy(out + at, s, n);
            at += n, s += n;
            if (ff) ++s;  // the stuffed zero
        }
        bits[j] = (uint32_t)(at * 8) - bit0[j];
    }
    while (at & 3) out[at++] = 0;
    memset(out + at, 0, 8);
    const size_t stream_words = at / 4 + 2;
    lay.seg_bit0 = lay.words + stream_words, lay.seg_bits = lay.seg_bit0 + nseg, lay.seg_sub0 = lay.seg_bits + nseg;
    lay.sub_seg = lay.seg_sub0 + nseg;
    memcpy(buf + lay.seg_bit0, bit0.data(), nseg * 4);
    memcpy(buf + lay.seg_bits, bits.data(), nseg * 4);
    int32_t* sub0 = reinterpret_cast<int32_t*>(buf + lay.seg_sub0);
    int32_t* sub_seg = reinterpret_cast<int32_t*>(buf + lay.sub_seg);
    int32_t nsub = 0;
    for (size_t j = 0; j < nseg; ++j) {
        sub0[j] = nsub;
        const uint32_t n = bits[j] ? (bits[j] + (uint32_t)subseq_bits - 1) / (uint32_t)subseq_bits : 1;
        for (uint32_t k = 0; k < n; ++k) sub_seg[nsub++] = (int32_t)j;
    }
    sc.nsub = lay.nsub = nsub;
    lay.total = lay.sub_seg + (size_t)nsub;
    return lay;
}
// Sync rounds after which the decoder gives up: the give-up distance, or the subsequences of the longest segment -- a cold
// start further back than that does not exist, so by then the fixed point is reached and confirmed.
inline int32_t max_sync_rounds(const uint32_t* buf, const Layout& lay, int32_t subseq_bits) {
    const int32_t* sub0 = reinterpret_cast<const int32_t*>(buf + lay.seg_sub0);
    int32_t longest = 1;
    for (int32_t j = 0; j < lay.nseg; ++j) {
        const int32_t n = (j + 1 < lay.nseg ? sub0[j + 1] : lay.nsub) - sub0[j];
        if (n > longest) longest = n;
    }
    const int32_t allowed = rounds_allowed(subseq_bits);
    return allowed < longest ? allowed : longest;
}
inline Stream stream_of(const uint32_t* buf, const Layout& lay) {
    Stream st;
    st.tables = reinterpret_cast<const EntropyTables*>(buf);
    st.words = buf + lay.words;
    st.seg_bit0 = buf + lay.seg_bit0, st.seg_bits = buf + lay.seg_bits;
    st.seg_sub0 = reinterpret_cast<const int32_t*>(buf + lay.seg_sub0);
    st.sub_seg = reinterpret_cast<const int32_t*>(buf + lay.sub_seg);
    return st;
}

}  // namespace me_jpeg_entropy
