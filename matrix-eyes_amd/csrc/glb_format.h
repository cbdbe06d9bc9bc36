// The glTF 2.0 binary (.glb) mesh writer's layout, JSON text and per-unit routines (glb_format.hip runs them on the GPU,
// mesh_host_format.h on the host behind ME_GLB_HOST_FORMAT).  HIP-free: with ME_GLB_HOST defined the same text is plain
// C++ (tests/glb_format_host.cpp runs the whole file under the sanitizers without a GPU).
//
// The file: a 12-byte header ("glTF", 2, total length), one JSON chunk padded with spaces so that its payload's length
// is 4 mod 16, and -- unless the mesh is empty -- one BIN chunk whose payload therefore starts at a file offset that is
// a multiple of 16.  BIN holds, each at a multiple of 16 with zeros in the gap before the next:
//   positions  V x 3 LE f32 (x, -y, -z: the reference writers' sign flips, output.rs:450)
//   colours    V x (r, g, b, 255) u8        (ME_VERTEX_COLOR with a colour array)
//   or UVs     V x 2 LE f32, uv unchanged   (ME_VERTEX_TEXTURE)
//   indices    3F LE u32, the faces in the reference's emission order
// so BIN is a sequence of 16-byte UNITS and every store of the packer is one aligned 16-byte store: four positions are
// three units, four colours one, and the UVs and indices are 16-byte copies of `uv` and `faces`.  Only the file's last
// unit can be short (the index section ends on a multiple of 4, where BIN ends); a section's last unit carries the
// zeros of the gap behind it.  Nothing here rounds: negating an f32 flips its sign bit.
//
// The accessor bounds are exact: minima and maxima under the total order of sign_key() (-0 below +0, a NaN beyond the
// infinity of its sign, so any NaN becomes a bound and the file is refused), which no reduction order can change.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "ryu_f64.h"

#if !defined(__HIPCC__) && !defined(ME_GLB_HOST)
#define ME_GLB_HOST 1   // a host compiler has no other mode
#endif
#ifdef ME_GLB_HOST
#define GLB_FN inline
#else
#define GLB_FN __host__ __device__ __forceinline__
#endif

namespace me_glb {

constexpr int kThreads = 256;
constexpr int64_t kMaxFileBytes = (int64_t)1 << 32;   // the header's length field is a u32

// what stands in section 2
enum Second { kNone = 0, kColors = 1, kUvs = 2 };

GLB_FN int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
GLB_FN int64_t units_of(int64_t bytes) { return (bytes + 15) >> 4; }

// Byte offsets within BIN and its length, in closed form
struct Layout {
    int64_t nverts, nfaces;
    int second;
    int64_t pos_bytes, second_off, second_bytes, index_off, index_bytes, bin_bytes;
};
GLB_FN Layout layout_of(int64_t nverts, int64_t nfaces, int second) {
    Layout l;
    l.nverts = nverts, l.nfaces = nfaces, l.second = second;
    l.pos_bytes = nverts * 12;
    l.second_off = align16(l.pos_bytes);
    l.second_bytes = second == kColors ? nverts * 4 : second == kUvs ? nverts * 8 : 0;
    l.index_off = align16(l.second_off + l.second_bytes);
    l.index_bytes = nfaces * 12;
    l.bin_bytes = (l.index_off + l.index_bytes + 3) & ~(int64_t)3;
    return l;
}
// the JSON chunk's payload: json_bytes of text and spaces up to the next length that is 4 mod 16
GLB_FN int64_t padded_json_bytes(int64_t json_bytes) { return align16(json_bytes + 12) - 12; }
// header + JSON chunk [+ BIN chunk header]: where BIN's payload starts, a multiple of 16
GLB_FN int64_t front_bytes(int64_t json_bytes, bool empty) { return 12 + 8 + padded_json_bytes(json_bytes) + (empty ? 0 : 8); }
GLB_FN int64_t file_bytes(const Layout& l, int64_t json_bytes) {
    return front_bytes(json_bytes, l.nverts == 0) + (l.nverts == 0 ? 0 : l.bin_bytes);
}

// An order-preserving integer image of an f32's bits, and back: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
GLB_FN int32_t sign_key(uint32_t bits) {
    const int32_t i = (int32_t)bits;
    return i ^ ((i >> 31) & 0x7fffffff);
}
GLB_FN uint32_t key_bits(int32_t key) { return (uint32_t)(key ^ ((key >> 31) & 0x7fffffff)); }

// Position unit q holds the f32 elements 4q .. 4q + 3 of xyz; element e is component e % 3, and the components 1 and 2
// (y, z) are written negated.  The mask of the unit's four elements follows q % 3 alone.
GLB_FN uint32_t flip_mask(int64_t q, int k) {
    const int c = (int)((q % 3 + k) % 3);
    return c ? 0x80000000u : 0u;
}
// the position triple of vertex i as it is written
GLB_FN void position_triple(const float* xyz, int64_t i, uint32_t out[3]) {
    memcpy(out, xyz + 3 * i, 12);
    out[1] ^= 0x80000000u, out[2] ^= 0x80000000u;
}
// r g b -> the little-endian word of (r, g, b, 255)
GLB_FN uint32_t rgba_word(const uint8_t* rgb) {
    return (uint32_t)rgb[0] | (uint32_t)rgb[1] << 8 | (uint32_t)rgb[2] << 16 | 0xff000000u;
}

struct PackArgs {
    const float* xyz;        // [nverts][3]
    const float* uv;         // [nverts][2], read when l.second == kUvs
    const uint8_t* rgb;      // per vertex id [nverts][3] at a multiple of 4, read when l.second == kColors
    const int32_t* faces;    // [nfaces][3] vertex ids
    Layout l;
    uint8_t* bin;            // BIN's payload, 16-byte aligned
};

GLB_FN int64_t total_units(const Layout& l) { return units_of(l.bin_bytes); }

#ifdef ME_GLB_HOST
GLB_FN void load16(const void* src, uint32_t w[4]) { memcpy(w, src, 16); }
GLB_FN void store16(uint8_t* dst, const uint32_t w[4]) { memcpy(dst, w, 16); }
GLB_FN void load12(const uint8_t* src, uint32_t x[3]) { memcpy(x, src, 12); }
#else
GLB_FN void load12(const uint8_t* src, uint32_t x[3]) {   // src: a multiple of 4
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src);
    x[0] = p[0], x[1] = p[1], x[2] = p[2];
}
GLB_FN void load16(const void* src, uint32_t w[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(src);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}
GLB_FN void store16(uint8_t* dst, const uint32_t w[4]) { *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]); }
#endif

// Words [4u, 4u + 4) of an array of `words` u32 at `src` (16-byte aligned): one 16-byte load where all four exist,
// zeros behind the array's end
GLB_FN void load_words(const void* src, int64_t u, int64_t words, uint32_t w[4]) {
    const uint32_t* p = (const uint32_t*)src + 4 * u;
    if (4 * u + 4 <= words) {
        load16(p, w);
    } else {
        for (int k = 0; k < 4; ++k) w[k] = 4 * u + k < words ? p[k] : 0u;
    }
}

// Unit u of BIN, u in [0, total_units): one aligned 16-byte store (the file's last unit: its words inside BIN)
GLB_FN void pack_unit(const PackArgs& a, int64_t u) {
    const Layout& l = a.l;
    uint32_t w[4];
    const int64_t at = 16 * u;
    if (at < l.second_off) {   // positions
        load_words(a.xyz, u, 3 * l.nverts, w);
        for (int k = 0; k < 4; ++k) w[k] = 4 * u + k < 3 * l.nverts ? w[k] ^ flip_mask(u, k) : 0u;
    } else if (at < l.index_off) {
        const int64_t s = u - (l.second_off >> 4);
        if (l.second == kUvs) {
            load_words(a.uv, s, 2 * l.nverts, w);
        } else if (4 * s + 4 <= l.nverts) {   // four colours: twelve bytes at a multiple of 4, as three words
            uint32_t x[3];
            load12(a.rgb + 12 * s, x);
            w[0] = x[0] | 0xff000000u;
            w[1] = x[0] >> 24 | x[1] << 8 | 0xff000000u;
            w[2] = x[1] >> 16 | x[2] << 16 | 0xff000000u;
            w[3] = x[2] >> 8 | 0xff000000u;
        } else {
            for (int k = 0; k < 4; ++k) w[k] = 4 * s + k < l.nverts ? rgba_word(a.rgb + 3 * (4 * s + k)) : 0u;
        }
    } else {
        load_words(a.faces, u - (l.index_off >> 4), 3 * l.nfaces, w);
    }
    if (at + 16 <= l.bin_bytes) {
        store16(a.bin + at, w);
    } else {
        for (int k = 0; at + 4 * k < l.bin_bytes; ++k) reinterpret_cast<uint32_t*>(a.bin + at)[k] = w[k];
    }
}

// The bounds of the written components as sign keys: key[0..2] minima of x, -y, -z, key[3..5] maxima
constexpr int32_t kKeyMax = 0x7fffffff, kKeyMin = -0x7fffffff - 1;
GLB_FN void bounds_identity(int32_t key[6]) {
    for (int c = 0; c < 3; ++c) key[c] = kKeyMax, key[3 + c] = kKeyMin;
}
GLB_FN void bounds_add_vertex(const float* xyz, int64_t i, int32_t key[6]) {
    uint32_t p[3];
    position_triple(xyz, i, p);
    for (int c = 0; c < 3; ++c) {
        const int32_t k = sign_key(p[c]);
        key[c] = k < key[c] ? k : key[c];
        key[3 + c] = k > key[3 + c] ? k : key[3 + c];
    }
}

// ---- host code: the JSON text --------------------------------------------------------------------------------------

// every key is an f32 that is finite (exponent field below 255)?
inline bool bounds_finite(const int32_t key[6]) {
    for (int c = 0; c < 6; ++c)
        if ((key_bits(key[c]) & 0x7f800000u) == 0x7f800000u) return false;
    return true;
}

// the f32 widened to f64 in the text of an OBJ "v" line (Rust's `{}`)
inline void append_number(std::string& s, int32_t key) {
    const uint32_t bits = key_bits(key);
    float f;
    memcpy(&f, &bits, 4);
    char text[me::ryu::kMaxFixedChars];
    s.append(text, (size_t)me::ryu::format_fixed((double)f, text));
}

// `"`, `\` and control bytes escaped (\u00xx, lower-case hex); every other byte, UTF-8 included, as it is
inline void append_json_string(std::string& s, const char* text) {
    static const char hex[] = "0123456789abcdef";
    s += '"';
    for (const unsigned char* p = (const unsigned char*)text; *p; ++p) {
        if (*p == '"' || *p == '\\') {
            s += '\\', s += (char)*p;
        } else if (*p < 0x20) {
            s += "\\u00", s += hex[*p >> 4], s += hex[*p & 15];
        } else {
            s += (char)*p;
        }
    }
    s += '"';
}

inline void append_view(std::string& s, int64_t off, int64_t bytes, int target) {
    s += "{\"buffer\":0,\"byteOffset\":" + std::to_string(off) + ",\"byteLength\":" + std::to_string(bytes) +
         ",\"target\":" + std::to_string(target) + "}";
}

// The JSON chunk's text, unpadded.  texture: ME_VERTEX_TEXTURE (the material names the source picture); bounds: the
// keys of the position accessor's min / max, read when the mesh is not empty.
inline std::string json_text(const Layout& l, bool texture, const char* source_path, const int32_t bounds[6]) {
    std::string s = "{\"asset\":{\"version\":\"2.0\",\"generator\":\"Matrix Eyes 3D surface\"},\"scene\":0,";
    if (l.nverts == 0) return s + "\"scenes\":[{\"nodes\":[]}]}";
    const int index_accessor = l.second == kNone ? 1 : 2;
    s += "\"scenes\":[{\"nodes\":[0]}],\"nodes\":[{\"mesh\":0}],\"meshes\":[{\"primitives\":[{\"attributes\":{\"POSITION\":0";
    if (l.second == kColors) s += ",\"COLOR_0\":1";
    if (l.second == kUvs) s += ",\"TEXCOORD_0\":1";
    s += "},\"indices\":" + std::to_string(index_accessor) + ",\"material\":0,\"mode\":4}]}],";
    s += "\"materials\":[{\"pbrMetallicRoughness\":{\"metallicFactor\":0,\"roughnessFactor\":1";
    if (texture) s += ",\"baseColorTexture\":{\"index\":0}";
    s += "},\"doubleSided\":true}],";
    if (texture) {
        s += "\"textures\":[{\"source\":0}],\"images\":[{\"uri\":";
        append_json_string(s, source_path);
        s += "}],";
    }
    s += "\"buffers\":[{\"byteLength\":" + std::to_string(l.bin_bytes) + "}],\"bufferViews\":[";
    append_view(s, 0, l.pos_bytes, 34962);
    if (l.second != kNone) s += ',', append_view(s, l.second_off, l.second_bytes, 34962);
    s += ',', append_view(s, l.index_off, l.index_bytes, 34963);
    const std::string count = std::to_string(l.nverts);
    s += "],\"accessors\":[{\"bufferView\":0,\"componentType\":5126,\"count\":" + count + ",\"type\":\"VEC3\",\"min\":[";
    for (int c = 0; c < 3; ++c) s += c ? "," : "", append_number(s, bounds[c]);
    s += "],\"max\":[";
    for (int c = 0; c < 3; ++c) s += c ? "," : "", append_number(s, bounds[3 + c]);
    s += "]}";
    if (l.second == kColors) s += ",{\"bufferView\":1,\"componentType\":5121,\"normalized\":true,\"count\":" + count + ",\"type\":\"VEC4\"}";
    if (l.second == kUvs) s += ",{\"bufferView\":1,\"componentType\":5126,\"count\":" + count + ",\"type\":\"VEC2\"}";
    s += ",{\"bufferView\":" + std::to_string(index_accessor) + ",\"componentType\":5125,\"count\":" + std::to_string(3 * l.nfaces) +
         ",\"type\":\"SCALAR\"}]}";
    return s;
}

inline void append_le32(std::string& s, uint32_t v) {
    const char b[4] = {(char)(v & 255), (char)(v >> 8 & 255), (char)(v >> 16 & 255), (char)(v >> 24)};
    s.append(b, 4);
}

// Everything in front of BIN's payload: the file header, the JSON chunk and, for a mesh that is not empty, the BIN
// chunk's header.  The caller has checked file_bytes() < kMaxFileBytes.
inline std::string front_text(const Layout& l, const std::string& json) {
    const int64_t padded = padded_json_bytes((int64_t)json.size());
    std::string s = "glTF";
    append_le32(s, 2);
    append_le32(s, (uint32_t)file_bytes(l, (int64_t)json.size()));
    append_le32(s, (uint32_t)padded);
    s += "JSON";
    s += json;
    s.append((size_t)(padded - (int64_t)json.size()), ' ');
    if (l.nverts) {
        append_le32(s, (uint32_t)l.bin_bytes);
        s.append("BIN\0", 4);
    }
    return s;
}

}  // namespace me_glb
