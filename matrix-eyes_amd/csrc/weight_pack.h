// Packing of checkpoint tensors into the weight arena, and the header of the arena cache file: the conversions, the index
// maps of the five PackKinds, the host packer and the cache header's reader and writer as plain functions.  The same text
// is the body of the pack kernels (weight_pack.hip: one thread per destination element or per tile lane) and, with
// ME_PACK_HOST defined, plain C++ without any HIP header (tests/weight_pack_host.cpp drives the index maps lane by lane
// against the host packer, and the header checks, under the sanitizers), in the style of jpeg_entropy.h and png_chunk.h.
//
// Conversions are integer arithmetic on the bit patterns, so that host and device agree bit for bit whatever the
// compiler or the device's denormal mode: float_to_half is round to nearest even (the bits of (_Float16)f for every
// input that is not a NaN), float_to_bf16 the rule weights.hip always had, an f64 source goes through (float) first
// (the double rounding is part of the contract), an f16 source into an f16 arena keeps its bits.  A NaN stays a NaN.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(ME_PACK_HOST) || !defined(__HIPCC__)
#define WP_FN inline
#else
#define WP_FN __host__ __device__ inline
#endif

namespace me_pack {

// mirrors of me::PackKind (model.h) and ME_WEIGHT_* / ME_DTYPE_* (matrix_eyes_hip.h): this header includes neither
enum : int32_t { K_VEC_F32 = 0, K_MAT_16 = 1, K_CONV_16 = 2, K_CONVT_16 = 3, K_CONVK_F32 = 4 };
enum : int32_t { W_F32 = 0, W_F16 = 1, W_BF16 = 2, W_F64 = 3 };
enum : int32_t { D_F16 = 0, D_BF16 = 1 };

// tiles of the two transposing kernels: kTileCi input channels (the contiguous axis of the destination) against kTileCo
// output channels of a ConvTranspose, or against the kh * kw taps of one output channel of a Conv (at most kMaxTaps)
constexpr int kTileCi = 64, kTileCo = 16, kMaxTaps = 64;
// row pitch of the LDS tile in 16-bit elements: 66 halfwords = 33 words, odd, so that a column walk (the load side writes
// one source run across rows) and a row walk (the store side) both spread over the banks
constexpr int kTilePitch = kTileCi + 2;

WP_FN uint32_t f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
WP_FN float bits_f32(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// IEEE half -> float, exact
WP_FN float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000) << 16;
    uint32_t exp = (h >> 10) & 0x1f, man = h & 0x3ff;
    uint32_t bits;
    if (exp == 0) {
        if (man == 0) {
            bits = sign;
        } else {
            int e = -1;
            do {
                ++e;
                man <<= 1;
            } while (!(man & 0x400));
            bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ff) << 13);
        }
    } else if (exp == 31) {
        bits = sign | 0x7f800000u | (man << 13);
    } else {
        bits = sign | ((exp + 127 - 15) << 23) | (man << 13);
    }
    return bits_f32(bits);
}

// float -> IEEE half, round to nearest even
WP_FN uint16_t float_to_half(float f) {
    uint32_t u = f32_bits(f);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000);
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00);   // NaN
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00);  // 65520 and beyond (inf included) round to inf
    if (u >= 0x38800000u) {                                  // a normal half: rebias, round the 13 bits that go
        const uint32_t v = u - 0x38000000u;
        return (uint16_t)(sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13));
    }
    if (u < 0x33000000u) return sign;                        // below 2^-25 (and 2^-25 itself, a tie to even): zero
    // a subnormal half: m * 2^(e - 150) in units of 2^-24
    const uint32_t e = u >> 23, m = (u & 0x7fffffu) | 0x800000u;
    const uint32_t shift = 126u - e;                         // 14 .. 24
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
}

WP_FN uint16_t float_to_bf16(float f) {
    const uint32_t u = f32_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1)) >> 16);
}

WP_FN size_t src_elem_size(int32_t dt) { return dt == W_F32 ? 4 : (dt == W_F64 ? 8 : 2); }

// element i of a source tensor as f32 (HostSrc::get of weights.hip)
WP_FN float src_get(const void* p, int32_t dt, int64_t i) {
    switch (dt) {
        case W_F32: return ((const float*)p)[i];
        case W_F16: return half_to_float(((const uint16_t*)p)[i]);
        case W_BF16: return bits_f32((uint32_t)((const uint16_t*)p)[i] << 16);
        default: return (float)((const double*)p)[i];
    }
}
// ... as the arena's 16-bit operand
WP_FN uint16_t src_get16(const void* p, int32_t dt, int64_t i, int32_t dst_dtype) {
    if (dst_dtype == D_F16 && dt == W_F16) return ((const uint16_t*)p)[i];  // fp16 checkpoint, f16 operands: exact
    const float f = src_get(p, dt, i);
    return dst_dtype == D_BF16 ? float_to_bf16(f) : float_to_half(f);
}
// ... as the bits of the arena's f32 (an f32 source keeps its bits, NaN payloads included)
WP_FN uint32_t src_get32(const void* p, int32_t dt, int64_t i) {
    if (dt == W_F32) return ((const uint32_t*)p)[i];
    return f32_bits(src_get(p, dt, i));
}

// The shape of one packing job, derived from (kind, dup, dims): what every index map below reads.
struct Shape {
    int32_t kind = 0;
    int32_t D = 1;             // 2: every run of K (or Cin) values is followed by a copy of itself, [W | W]
    int64_t numel = 0;         // source elements
    int64_t N = 0, K = 0;      // K_MAT_16: rows and row length
    int64_t Cout = 0, Cin = 0; // K_CONV_16, K_CONVT_16, K_CONVK_F32 (Cin only)
    int64_t kk = 0;            // taps: kh * kw (K_CONV_16, K_CONVK_F32), 4 (K_CONVT_16)
    int64_t dst_elems = 0;     // destination elements (16-bit or f32)
    int64_t dst_bytes = 0;
};

// 0, or why (dims, ndim) is not a tensor of `kind`
WP_FN const char* make_shape(int32_t kind, int32_t dup, const int64_t* dims, int32_t ndim, Shape* out) {
    if (!dims || ndim < 1 || ndim > 4) return "1 to 4 dimensions";
    Shape s;
    s.kind = kind;
    s.numel = 1;
    for (int i = 0; i < ndim; ++i) {
        if (dims[i] <= 0 || dims[i] > ((int64_t)1 << 31)) return "every dimension in [1, 2^31]";
        s.numel *= dims[i];
        if (s.numel > ((int64_t)1 << 38)) return "at most 2^38 elements";
    }
    const bool f32 = kind == K_VEC_F32 || kind == K_CONVK_F32;
    s.D = dup && !f32 ? 2 : 1;
    switch (kind) {
        case K_VEC_F32: break;
        case K_MAT_16: s.N = dims[0], s.K = s.numel / s.N; break;
        case K_CONV_16:
            if (ndim != 4) return "a Conv2d weight has 4 dimensions";
            s.Cout = dims[0], s.Cin = dims[1], s.kk = dims[2] * dims[3];
            if (s.kk > kMaxTaps) return "at most 64 taps";
            break;
        case K_CONVT_16:
            if (ndim != 4 || dims[2] != 2 || dims[3] != 2) return "a ConvTranspose2d weight is [Cin][Cout][2][2]";
            s.Cin = dims[0], s.Cout = dims[1], s.kk = 4;
            break;
        case K_CONVK_F32:
            if (ndim != 4 || dims[0] != 1) return "[1][Cin][k][k]";
            s.Cin = dims[1], s.kk = dims[2] * dims[3];
            break;
        default: return "unknown pack kind";
    }
    s.dst_elems = s.numel * s.D;
    s.dst_bytes = s.dst_elems * (f32 ? 4 : 2);
    *out = s;
    return nullptr;
}

// Destination-major index map: the source element that destination element `d` holds.
//   K_VEC_F32    d
//   K_MAT_16     [N][D * K]              <- [N][K]
//   K_CONV_16    [Cout][kk][D * Cin]     <- [Cout][Cin][kk]
//   K_CONVT_16   [(q * Cout + co)][D * Cin] <- [Cin][Cout][q]
//   K_CONVK_F32  [kk][Cin]               <- [Cin][kk]
WP_FN int64_t src_index(const Shape& s, int64_t d) {
    switch (s.kind) {
        case K_MAT_16: {
            if (s.D == 1) return d;
            const int64_t r = d / (2 * s.K), c = d % (2 * s.K);
            return r * s.K + (c >= s.K ? c - s.K : c);
        }
        case K_CONV_16: {
            const int64_t w = s.D * s.Cin, row = d / w, c = d % w;  // row = co * kk + t
            const int64_t ci = c >= s.Cin ? c - s.Cin : c, co = row / s.kk, t = row % s.kk;
            return (co * s.Cin + ci) * s.kk + t;
        }
        case K_CONVT_16: {
            const int64_t w = s.D * s.Cin, row = d / w, c = d % w;  // row = q * Cout + co
            const int64_t ci = c >= s.Cin ? c - s.Cin : c, q = row / s.Cout, co = row % s.Cout;
            return (ci * s.Cout + co) * 4 + q;
        }
        case K_CONVK_F32: {
            const int64_t t = d / s.Cin, ci = d % s.Cin;
            return ci * s.kk + t;
        }
        default: return d;
    }
}

// ---- the two transposing kernels, work item by work item ----------------------------------------------------------------
// A workgroup of kTileThreads lanes owns one tile; lane t does work items t, t + kTileThreads, ... of the load phase (a
// source element into the LDS tile), the workgroup synchronises, and likewise for the store phase (an LDS element to the
// destination).  The functions below say which elements work item i touches: the kernels and the host twin run the same text.
constexpr int kTileThreads = 256;
struct TileRef {
    int lds;      // element of the LDS tile
    int64_t g;    // element of the source (load phase) or of the destination (store phase)
};
WP_FN int tile_nci(const Shape& s, int64_t bx) { return (int)(s.Cin - bx * kTileCi < kTileCi ? s.Cin - bx * kTileCi : kTileCi); }

// K_CONV_16: tile (bx, by) = input channels [bx * kTileCi, +nci) of output channel by; LDS [kk][kTilePitch]
WP_FN int conv_tile_loads(const Shape& s, int64_t bx) { return tile_nci(s, bx) * (int)s.kk; }
WP_FN TileRef conv_tile_load(const Shape& s, int64_t bx, int64_t by, int i) {
    const int kk = (int)s.kk, ci = i / kk, t = i - ci * kk;
    return TileRef{t * kTilePitch + ci, (by * s.Cin + bx * kTileCi) * kk + i};   // nci * kk contiguous source elements
}
WP_FN int conv_tile_stores(const Shape& s) { return (int)s.kk * s.D * kTileCi; }
WP_FN bool conv_tile_store(const Shape& s, int64_t bx, int64_t by, int i, TileRef* out) {
    const int r = i / kTileCi, ci = i % kTileCi;
    if (ci >= tile_nci(s, bx)) return false;
    const int t = r / s.D, d = r - t * s.D;
    *out = TileRef{t * kTilePitch + ci, ((by * s.kk + t) * s.D + d) * s.Cin + bx * kTileCi + ci};
    return true;
}

// K_CONVT_16: tile (bx, by) = input channels [bx * kTileCi, +nci) x output channels [by * kTileCo, +nco); LDS [4][kTileCo][kTilePitch]
WP_FN int tile_nco(const Shape& s, int64_t by) { return (int)(s.Cout - by * kTileCo < kTileCo ? s.Cout - by * kTileCo : kTileCo); }
WP_FN int convt_tile_loads(const Shape& s, int64_t bx, int64_t by) { return tile_nci(s, bx) * tile_nco(s, by) * 4; }
WP_FN TileRef convt_tile_load(const Shape& s, int64_t bx, int64_t by, int i) {
    const int run = tile_nco(s, by) * 4;   // contiguous source elements per input channel: [co][q]
    const int ci = i / run, r = i - ci * run, co = r >> 2, q = r & 3;
    return TileRef{(q * kTileCo + co) * kTilePitch + ci, ((bx * kTileCi + ci) * s.Cout + by * kTileCo) * 4 + r};
}
WP_FN int convt_tile_stores(const Shape& s, int64_t by) { return 4 * tile_nco(s, by) * s.D * kTileCi; }
WP_FN bool convt_tile_store(const Shape& s, int64_t bx, int64_t by, int i, TileRef* out) {
    const int r = i / kTileCi, ci = i % kTileCi;
    if (ci >= tile_nci(s, bx)) return false;
    const int nco = tile_nco(s, by), rc = r / s.D, d = r - rc * s.D, q = rc / nco, co = rc - q * nco;
    *out = TileRef{(q * kTileCo + co) * kTilePitch + ci, ((q * s.Cout + by * kTileCo + co) * s.D + d) * s.Cin + bx * kTileCi + ci};
    return true;
}
// The store phase eight input channels at a time (one 16-byte store per work item), when every destination row starts on a
// 16-byte boundary: work item i of that form is the scalar work item of its first channel.
WP_FN bool tile_store8_ok(const Shape& s) { return s.Cin % 8 == 0; }
WP_FN int tile_store8_item(int i) { return (i >> 3) * kTileCi + (i & 7) * 8; }
constexpr int kConvTileElems = kMaxTaps * kTilePitch, kConvtTileElems = 4 * kTileCo * kTilePitch;

// ---- the checksum of the cache file's payload ------------------------------------------------------------------------
// The sum over the arena's 32-bit words of a mixed (position, word) term, modulo 2^64: integer addition commutes, so the
// device's block sums and atomic adds give the same value in any order, on every run.
WP_FN uint64_t checksum_term(uint64_t index, uint32_t word) {
    uint64_t x = (index << 32) ^ (index >> 32) ^ (uint64_t)word ^ 0x9e3779b97f4a7c15ull;
    x ^= x >> 33, x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33, x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// ---- the host packer: the loops of load_weight, source-major ----------------------------------------------------------
inline void pack_host(const Shape& s, int32_t dst_dtype, const void* data, int32_t weight_dtype, void* packed) {
    const int64_t n = s.numel;
    uint16_t* o16 = reinterpret_cast<uint16_t*>(packed);
    auto put16 = [&](int64_t dst, int64_t si) { o16[dst] = src_get16(data, weight_dtype, si, dst_dtype); };
    switch (s.kind) {
        case K_VEC_F32: {
            uint32_t* o = reinterpret_cast<uint32_t*>(packed);
            if (weight_dtype == W_F32)
                memcpy(o, data, (size_t)n * 4);
            else
                for (int64_t i = 0; i < n; ++i) o[i] = src_get32(data, weight_dtype, i);
            break;
        }
        // dup: every run of K (or Cin) source values is followed by a copy of itself: [W | W]
        case K_MAT_16:
            if (s.D == 2) {
                const int64_t N = s.N, K = s.K;
                for (int64_t r = 0; r < N; ++r)
                    for (int64_t k = 0; k < K; ++k) put16(r * 2 * K + k, r * K + k), put16(r * 2 * K + K + k, r * K + k);
            } else if (dst_dtype == D_F16 && weight_dtype == W_F16) {
                memcpy(packed, data, (size_t)n * 2);
            } else {
                for (int64_t i = 0; i < n; ++i) put16(i, i);
            }
            break;
        case K_CONV_16: {  // [Cout][Cin][kh][kw] -> [Cout][kh*kw][Cin]
            const int64_t Cout = s.Cout, Cin = s.Cin, kk = s.kk, D = s.D;
            for (int64_t co = 0; co < Cout; ++co)
                for (int64_t ci = 0; ci < Cin; ++ci)
                    for (int64_t t = 0; t < kk; ++t)
                        for (int64_t d = 0; d < D; ++d)
                            put16((co * kk + t) * D * Cin + d * Cin + ci, (co * Cin + ci) * kk + t);
            break;
        }
        case K_CONVT_16: {  // [Cin][Cout][2][2] -> [(dy*2+dx)*Cout + co][Cin]
            const int64_t Cin = s.Cin, Cout = s.Cout, D = s.D;
            for (int64_t ci = 0; ci < Cin; ++ci)
                for (int64_t co = 0; co < Cout; ++co)
                    for (int64_t q = 0; q < 4; ++q)
                        for (int64_t d = 0; d < D; ++d)
                            put16((q * Cout + co) * D * Cin + d * Cin + ci, (ci * Cout + co) * 4 + q);
            break;
        }
        case K_CONVK_F32: {  // [1][Cin][k][k] -> f32 [k][k][Cin]
            const int64_t Cin = s.Cin, kk = s.kk;
            uint32_t* o = reinterpret_cast<uint32_t*>(packed);
            for (int64_t ci = 0; ci < Cin; ++ci)
                for (int64_t t = 0; t < kk; ++t) o[t * Cin + ci] = src_get32(data, weight_dtype, ci * kk + t);
            break;
        }
    }
}

// ---- the cache file: one fixed-size header, then the raw arena ---------------------------------------------------------
// Bumped by whoever changes what a packed or composed slot holds for the same checkpoint and layout.
constexpr uint32_t ME_ARENA_FORMAT = 1;
constexpr size_t kArenaHeaderBytes = 256;
constexpr int kArenaConfigWords = 17;   // sizeof(me_model_config) / 4

struct ArenaHeader {
    char magic[8];                       // "MEARENA\0"
    uint32_t format;                     // ME_ARENA_FORMAT
    uint32_t header_bytes;               // kArenaHeaderBytes
    int32_t dtype;                       // the context's ME_DTYPE_* as created (fp8 included)
    int32_t split_mask;
    uint32_t config[kArenaConfigWords];  // me_model_config, word for word
    uint32_t reserved0;
    uint64_t layout;                     // me_weight_arena_layout
    uint64_t arena_bytes;
    int64_t source_size;                 // of the checkpoint the arena was packed from; -1: not recorded
    int64_t source_mtime_ns;
    uint64_t checksum;                   // of the payload (checksum_term summed over its words)
    uint8_t pad[kArenaHeaderBytes - 8 - 4 * 4 - 4 * kArenaConfigWords - 4 - 8 * 5];
};
static_assert(sizeof(ArenaHeader) == kArenaHeaderBytes, "the cache header is 256 bytes");

// what this context expects of a cache file
struct ArenaExpect {
    int32_t dtype = 0, split_mask = 0;
    uint32_t config[kArenaConfigWords] = {};
    uint64_t layout = 0, arena_bytes = 0;
};

inline void arena_header_write(const ArenaExpect& e, int64_t source_size, int64_t source_mtime_ns, uint64_t checksum,
                               void* out256) {
    ArenaHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "MEARENA", 8);
    h.format = ME_ARENA_FORMAT, h.header_bytes = (uint32_t)kArenaHeaderBytes;
    h.dtype = e.dtype, h.split_mask = e.split_mask;
    memcpy(h.config, e.config, sizeof h.config);
    h.layout = e.layout, h.arena_bytes = e.arena_bytes;
    h.source_size = source_size, h.source_mtime_ns = source_mtime_ns;
    h.checksum = checksum;
    memcpy(out256, &h, sizeof h);
}

enum ArenaVerdict : int32_t {
    ARENA_OK = 0,
    ARENA_STALE_FORMAT = 1,   // written under another ME_ARENA_FORMAT: not an error, the checkpoint is loaded instead
    ARENA_STALE_SOURCE = 2,   // written for a checkpoint of another size or mtime: likewise
    ARENA_SHORT = 10,         // everything from here on is damage
    ARENA_BAD_MAGIC = 11,
    ARENA_BAD_HEADER = 12,
    ARENA_OTHER_CONTEXT = 13, // dtype, configuration, split mask, layout hash or size are not this context's
    ARENA_BAD_SIZE = 14,      // the file is not header + payload long
};

// The verdict on the first `have` bytes of a file that is `file_bytes` long.  has_source: the checkpoint exists, with
// this size and mtime; without it the recorded stamp is not looked at.  *out receives the header when there is one.
inline ArenaVerdict arena_header_check(const void* head, size_t have, uint64_t file_bytes, const ArenaExpect& e,
                                       bool has_source, int64_t source_size, int64_t source_mtime_ns, ArenaHeader* out) {
    if (have < kArenaHeaderBytes || file_bytes < kArenaHeaderBytes) return ARENA_SHORT;
    ArenaHeader h;
    memcpy(&h, head, sizeof h);
    if (out) *out = h;
    if (memcmp(h.magic, "MEARENA", 8) != 0) return ARENA_BAD_MAGIC;
    if (h.header_bytes != kArenaHeaderBytes) return ARENA_BAD_HEADER;
    if (h.format != ME_ARENA_FORMAT) return ARENA_STALE_FORMAT;
    if (h.dtype != e.dtype || h.split_mask != e.split_mask || memcmp(h.config, e.config, sizeof h.config) != 0 ||
        h.layout != e.layout || h.arena_bytes != e.arena_bytes)
        return ARENA_OTHER_CONTEXT;
    if (file_bytes != kArenaHeaderBytes + h.arena_bytes) return file_bytes < kArenaHeaderBytes + h.arena_bytes ? ARENA_SHORT : ARENA_BAD_SIZE;
    if (has_source && (h.source_size != source_size || h.source_mtime_ns != source_mtime_ns)) return ARENA_STALE_SOURCE;
    return ARENA_OK;
}

inline const char* arena_verdict_text(ArenaVerdict v) {
    switch (v) {
        case ARENA_OK: return "valid";
        case ARENA_STALE_FORMAT: return "written under another ME_ARENA_FORMAT";
        case ARENA_STALE_SOURCE: return "written for a checkpoint of another size or modification time";
        case ARENA_SHORT: return "the file is too short";
        case ARENA_BAD_MAGIC: return "not an arena cache (wrong magic)";
        case ARENA_BAD_HEADER: return "unreadable header";
        case ARENA_OTHER_CONTEXT: return "dtype, model configuration, split mask, layout hash or size are not this context's";
        case ARENA_BAD_SIZE: return "the file is longer than its header says";
    }
    return "?";
}

// <dir>/<stem>-<dtype>-<16 hex digits of the layout hash>.mearena beside `checkpoint_path`; the length written without the
// terminator, or -1 when cap is too small
inline int64_t arena_cache_path(const char* checkpoint_path, const char* dtype_name, uint64_t layout, char* buf, size_t cap) {
    const size_t len = strlen(checkpoint_path);
    size_t slash = len;   // index behind the last '/', 0 when none
    while (slash > 0 && checkpoint_path[slash - 1] != '/') --slash;
    size_t stem_end = len;   // the last '.' of the file name, unless it leads the name
    for (size_t i = len; i > slash + 1; --i)
        if (checkpoint_path[i - 1] == '.') {
            stem_end = i - 1;
            break;
        }
    static const char hex[] = "0123456789abcdef";
    char tail[16 + 1];
    for (int i = 0; i < 16; ++i) tail[i] = hex[(layout >> (60 - 4 * i)) & 15];
    tail[16] = 0;
    const size_t need = stem_end + 1 + strlen(dtype_name) + 1 + 16 + strlen(".mearena");
    if (!buf || need + 1 > cap) return -1;
    size_t o = 0;
    memcpy(buf, checkpoint_path, stem_end), o = stem_end;
    buf[o++] = '-';
    memcpy(buf + o, dtype_name, strlen(dtype_name)), o += strlen(dtype_name);
    buf[o++] = '-';
    memcpy(buf + o, tail, 16), o += 16;
    memcpy(buf + o, ".mearena", 9), o += 8;
    return (int64_t)o;
}

}  // namespace me_pack
