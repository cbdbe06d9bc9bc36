// The text of one OBJ line (reference src/output.rs:484-630 ObjWriter): what the kernels of obj_format.hip format into an
// LDS slot per thread and the host serialiser (mesh_host_format.h, the A/B behind ME_OBJ_HOST_FORMAT) into a stack buffer
// of the same size.  With ME_OBJ_HOST defined the same text is plain C++ (tests/mesh_format_host.cpp holds the slot
// sizes to the worst-case inputs without a GPU).  Nothing here depends on the unit's contraction flag: 1.0 - v and
// c / 255.0 are single f64 operations.
#pragma once
#include <stdint.h>

#include "ryu_f64.h"

#ifdef ME_OBJ_HOST
#define OBJ_FN inline
#define OBJ_ROLLED
#else
#define OBJ_FN __host__ __device__ __forceinline__
#define OBJ_ROLLED _Pragma("unroll 1")
#endif

namespace me {
// Internal linkage, as when this text stood in obj_format.hip: each including unit formats its own lines, and the kernels
// that take an ObjArgs keep their names.
namespace {

// Bytes of a line's slot = the longest line of each section.  A number that came from an f32 (every coordinate; 1 - v
// is an exact f64 difference of one) prints in at most 64 characters: sign, "0.", 44 zeros, 17 digits; a colour
// c / 255.0 in 20.
constexpr int kSlotVt = 136;   // "vt " + 64 + ' ' + 64 + '\n'
constexpr int kSlotV = 264;    // "v " + 3 x (64 + ' ') + 3 x (20 + ' ') + '\n'
constexpr int kSlotF = 72;     // 'f' + 3 x (' ' + 10 + '/' + 10) + '\n'

struct ObjArgs {
    const float* uv;         // [count][2]  (vt)
    const float* xyz;        // [count][3]  (v)
    const uint8_t* colors;   // per vertex id [count][3], or null
    const int32_t* faces;    // [count][3]  (f)
    int64_t count;           // lines of this section
    int tex;                 // f: "a/a" pairs
};

// line i of section SEC (0: vt, 1: v, 2: f) into `out`; returns its length, the '\n' included
template <int SEC>
OBJ_FN int format_line(const ObjArgs& a, int64_t i, char* out) {
    int n = 0;
    if constexpr (SEC == 0) {  // output.rs:592-602: vt u (1 - v), both widened to f64 first
        out[0] = 'v', out[1] = 't', out[2] = ' ';
        n = 3;
        n += ryu::format_fixed((double)a.uv[2 * i], out + n);
        out[n++] = ' ';
        n += ryu::format_fixed(1.0 - (double)a.uv[2 * i + 1], out + n);
    } else if constexpr (SEC == 1) {  // output.rs:566-590: v x -y -z [r g b]
        out[0] = 'v', out[1] = ' ';
        n = 2;
        n += ryu::format_fixed((double)a.xyz[3 * i], out + n);
        out[n++] = ' ';
        n += ryu::format_fixed((double)(-a.xyz[3 * i + 1]), out + n);
        out[n++] = ' ';
        n += ryu::format_fixed((double)(-a.xyz[3 * i + 2]), out + n);
        if (a.colors) {
            OBJ_ROLLED
            for (int c = 0; c < 3; ++c) {
                out[n++] = ' ';
                n += ryu::format_fixed((double)a.colors[3 * i + c] / 255.0, out + n);
            }
        }
    } else {  // output.rs:604-620: f a/a b/b c/c, 1-based
        out[0] = 'f';
        n = 1;
        OBJ_ROLLED
        for (int k = 0; k < 3; ++k) {
            const uint64_t idx = (uint64_t)a.faces[3 * i + k] + 1;
            out[n++] = ' ';
            n += ryu::format_u64(idx, out + n);
            if (a.tex) {
                out[n++] = '/';
                n += ryu::format_u64(idx, out + n);
            }
        }
    }
    out[n++] = '\n';
    return n;
}

}  // namespace
}  // namespace me
