// The per-record and per-workgroup routines of the binary PLY writer (ply_format.hip; reference src/output.rs:385-482
// PlyWriter): one vertex record, one face record, and the packing of one workgroup's records into the file.  Written
// as a sequence of PHASES -- PLY_LANES { code of lane t } PLY_SYNC -- like png_chunk.h, so that the same text is a HIP
// kernel body (a phase = the code of thread t, PLY_SYNC = __syncthreads) and, with ME_PLY_HOST defined, plain C++ that
// runs a phase lane by lane (tests/ply_format_host.cpp: the layout is checked without a GPU).
//
// The records have fixed sizes, so the file is closed-form: `body` bytes of ASCII header the caller writes itself, then
// nverts records of 24 bytes (x, -y, -z as big-endian f64) or 27 (+ r g b), then nfaces records of 13 bytes (the byte 3
// and three big-endian u32 vertex ids).  Neither section starts on a multiple of 16 and no record size divides 16, so a
// workgroup lays its kThreads records end to end in a staging area (LDS) at an offset congruent mod 16 to the address
// they go to, and copies them out as aligned 16-byte chunks; only the two ragged ends of its span are byte stores.
// Nothing here rounds: negating an f32 and widening it to f64 are exact.
#pragma once
#include <stdint.h>
#include <string.h>

namespace me_ply {

constexpr int kThreads = 256;        // lanes of a workgroup = records of a workgroup
constexpr int kVertexBytes = 24;     // three big-endian f64
constexpr int kColorBytes = 3;       // r g b behind them when colours are written
constexpr int kFaceBytes = 13;       // the count 3 + three big-endian u32
constexpr int kStageBytes = 16 + kThreads * (kVertexBytes + kColorBytes);   // misalignment <= 15, + the longest span

struct PackArgs {
    const float* xyz;        // [nverts][3]
    const uint8_t* rgb;      // per vertex id [nverts][3], or null: 24-byte vertex records
    const int32_t* faces;    // [nfaces][3] vertex ids
    int64_t nverts, nfaces;
    int64_t body;            // bytes in front of the first vertex record (the header)
    uint8_t* out;            // the file
};

#ifdef ME_PLY_HOST
#define PLY_FN inline
#define PLY_WG_FN inline
#define PLY_LANES for (int t = 0; t < ::me_ply::kThreads; ++t) {
#define PLY_SYNC }
// (the sanitizers see every byte that moves)
PLY_FN void copy16(uint8_t* dst, const uint8_t* src) { memcpy(dst, src, 16); }
#else
#define PLY_FN __host__ __device__ __forceinline__
#define PLY_WG_FN __device__ __forceinline__
#define PLY_LANES { const int t = (int)threadIdx.x;
#define PLY_SYNC } __syncthreads();
PLY_FN void copy16(uint8_t* dst, const uint8_t* src) { *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src); }
#endif

PLY_FN int64_t blocks_of(int64_t records) { return (records + kThreads - 1) / kThreads; }
PLY_FN int vertex_bytes(const PackArgs& a) { return a.rgb ? kVertexBytes + kColorBytes : kVertexBytes; }
PLY_FN int64_t file_bytes(const PackArgs& a) { return a.body + a.nverts * vertex_bytes(a) + a.nfaces * kFaceBytes; }

PLY_FN void put_be32(uint8_t* d, uint32_t u) {
    d[0] = (uint8_t)(u >> 24), d[1] = (uint8_t)(u >> 16), d[2] = (uint8_t)(u >> 8), d[3] = (uint8_t)u;
}
// f64::to_be_bytes of an f32 widened to f64
PLY_FN void put_be_f64(uint8_t* d, float v) {
    const double w = (double)v;
    uint64_t u;
    memcpy(&u, &w, 8);
    put_be32(d, (uint32_t)(u >> 32));
    put_be32(d + 4, (uint32_t)u);
}

// output.rs:440-458: x, -y, -z (negated as f32, then widened) and the vertex's colour
PLY_FN void vertex_record(const float* xyz, const uint8_t* rgb, int64_t i, uint8_t* d) {
    put_be_f64(d, xyz[3 * i]);
    put_be_f64(d + 8, -xyz[3 * i + 1]);
    put_be_f64(d + 16, -xyz[3 * i + 2]);
    if (rgb) {
        d[24] = rgb[3 * i], d[25] = rgb[3 * i + 1], d[26] = rgb[3 * i + 2];
    }
}

// output.rs:464-473
PLY_FN void face_record(const int32_t* faces, int64_t f, uint8_t* d) {
    d[0] = 3;
    put_be32(d + 1, (uint32_t)faces[3 * f]);
    put_be32(d + 5, (uint32_t)faces[3 * f + 1]);
    put_be32(d + 9, (uint32_t)faces[3 * f + 2]);
}

// The records of workgroup `block`: blocks [0, blocks_of(nverts)) hold vertices, the ones behind them faces.
struct Span {
    int64_t first;    // first record of the section
    int64_t at;       // where it goes, bytes from a.out
    int count;        // records, 1 .. kThreads
    int rec;          // bytes per record
    bool face;
};
PLY_FN Span span_of(const PackArgs& a, int64_t block) {
    const int64_t bv = blocks_of(a.nverts);
    Span s;
    s.face = block >= bv;
    s.first = (s.face ? block - bv : block) * kThreads;
    const int64_t left = (s.face ? a.nfaces : a.nverts) - s.first;
    s.count = (int)(left < kThreads ? left : kThreads);
    s.rec = s.face ? kFaceBytes : vertex_bytes(a);
    s.at = a.body + (s.face ? a.nverts * vertex_bytes(a) : 0) + s.first * s.rec;
    return s;
}

// One workgroup.  `stage`: kStageBytes of workgroup memory, 16-byte aligned.
PLY_WG_FN void pack_block(const PackArgs& a, int64_t block, uint8_t* stage) {
    const Span s = span_of(a, block);
    uint8_t* const dst = a.out + s.at;
    const int mis = (int)((uintptr_t)dst & 15);   // stage + mis + p holds byte p of the span: the same residue mod 16 as dst + p
    const int total = s.count * s.rec;
    PLY_LANES
        if (t < s.count) {
            uint8_t* d = stage + mis + t * s.rec;
            if (s.face) face_record(a.faces, s.first + t, d);
            else vertex_record(a.xyz, a.rgb, s.first + t, d);
        }
    PLY_SYNC
    PLY_LANES
        const int nchunks = (mis + total + 15) >> 4;
        for (int c = t; c < nchunks; c += kThreads) {
            const int start = 16 * c - mis;   // first byte of the chunk, relative to the span
            if (start >= 0 && start + 16 <= total) {
                copy16(dst + start, stage + 16 * c);
            } else {   // a ragged end: the bytes outside belong to a neighbouring workgroup, the header, or nobody
                for (int k = 0; k < 16; ++k) {
                    const int p = start + k;
                    if (p >= 0 && p < total) dst[p] = stage[16 * c + k];
                }
            }
        }
    PLY_SYNC
}

}  // namespace me_ply
