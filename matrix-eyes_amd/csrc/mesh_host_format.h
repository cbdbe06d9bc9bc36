// The mesh files serialised on the host (reference src/output.rs:385-630 PlyWriter, ObjWriter): the A/B of the device
// formatters (ME_OBJ_HOST_FORMAT, ME_PLY_HOST_FORMAT, ME_GLB_HOST_FORMAT; mesh_writer.hip write_host_mesh).  Every line,
// record and unit is the text the kernels run -- obj_format.h format_line, ply_format.h vertex_record / face_record,
// glb_format.h pack_unit -- so only the headers, the .mtl and the path rules are spelled out here.  Plain C++17:
// tests/mesh_format_host.cpp includes it with ME_OBJ_HOST and ME_PLY_HOST defined, tests/glb_format_host.cpp with
// ME_GLB_HOST too (glb_format.h is in host mode under any compiler but hipcc), and neither needs HIP.
#pragma once
#include <ctype.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "glb_format.h"
#include "obj_format.h"
#include "ply_format.h"

namespace me_mesh_host {

inline bool ends_with_ci(const std::string& s, const char* suffix) {
    const size_t n = strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (tolower((unsigned char)s[s.size() - n + i]) != suffix[i]) return false;
    return true;
}

// Path::file_stem / Path::parent for '/'-separated paths
inline std::string file_stem(const std::string& path) {
    const size_t slash = path.find_last_of('/');
    std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    const size_t dot = name.find_last_of('.');
    if (dot != std::string::npos && dot != 0) name = name.substr(0, dot);
    return name;
}
inline std::string parent_dir(const std::string& path) {
    const size_t slash = path.find_last_of('/');
    if (slash == std::string::npos) return "";
    return slash == 0 ? "/" : path.substr(0, slash);
}

// output.rs:556-562: the two lines in front of a textured OBJ; output.rs:525-547: the .mtl beside it and its text
inline std::string obj_header(const std::string& stem) { return "mtllib " + stem + ".mtl\nusemtl Textured\n"; }
inline std::string mtl_path(const std::string& dest) {
    const std::string dir = parent_dir(dest);
    return (dir.empty() ? std::string() : dir + "/") + file_stem(dest) + ".mtl";
}
inline std::string mtl_text(const std::string& source_path) {
    return "newmtl Textured\nKa 0.2 0.2 0.2\nKd 0.8 0.8 0.8\nKs 1.0 1.0 1.0\nillum 2\nNs 0.000500\nmap_Ka " + source_path +
           "\nmap_Kd " + source_path + "\n\n";
}

// output.rs:415-438: the ASCII header of a PLY file.  The colour properties follow the vertex MODE; whether the records
// carry colours follows the colour array (ME_VERTEX_COLOR without one: colour properties, 24-byte records).
inline std::string ply_header(int64_t nverts, int64_t nfaces, bool color_properties) {
    std::string b = "ply\nformat binary_big_endian 1.0\ncomment Matrix Eyes 3D surface\n";
    b += "element vertex " + std::to_string(nverts) + "\n";
    b += "property double x\nproperty double y\nproperty double z\n";
    if (color_properties) b += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    b += "element face " + std::to_string(nfaces) + "\n";
    b += "property list uchar int vertex_indices\nend_header\n";
    return b;
}

// Item i of a section, appended to `out` (the shape of me::AppendItem).  OBJ: args is the section's me::ObjArgs, the line
// goes through a buffer of the slot size the kernels give it.  PLY: args is the file's me_ply::PackArgs.
template <int SEC>
void append_obj_line(const void* args, int64_t i, std::string& out) {
    char line[SEC == 0 ? me::kSlotVt : SEC == 1 ? me::kSlotV : me::kSlotF];
    out.append(line, (size_t)me::format_line<SEC>(*(const me::ObjArgs*)args, i, line));
}
inline void append_ply_vertex(const void* args, int64_t i, std::string& out) {
    const me_ply::PackArgs& a = *(const me_ply::PackArgs*)args;
    uint8_t rec[me_ply::kVertexBytes + me_ply::kColorBytes];
    me_ply::vertex_record(a.xyz, a.rgb, i, rec);
    out.append((const char*)rec, (size_t)me_ply::vertex_bytes(a));
}
inline void append_ply_face(const void* args, int64_t f, std::string& out) {
    uint8_t rec[me_ply::kFaceBytes];
    me_ply::face_record(((const me_ply::PackArgs*)args)->faces, f, rec);
    out.append((const char*)rec, sizeof rec);
}

// The sections of each file in the reference's order: visit(count, item, args) once per section.  args point into the
// ObjSections / PackArgs, which therefore outlive whatever the visitor keeps.  (Internal linkage, as the ObjArgs it holds.)
namespace {
struct ObjSections {
    me::ObjArgs vt, v, f;
    ObjSections(const float* uv, const float* xyz, const uint8_t* colors, const int32_t* faces, int64_t nverts, int64_t nfaces,
                bool tex)
        : vt{uv, nullptr, nullptr, nullptr, tex ? nverts : 0, 0}, v{nullptr, xyz, colors, nullptr, nverts, 0},
          f{nullptr, nullptr, nullptr, faces, nfaces, tex ? 1 : 0} {}
    template <typename Visit>
    void each(Visit&& visit) const {
        if (f.tex) visit(vt.count, &append_obj_line<0>, (const void*)&vt);
        visit(v.count, &append_obj_line<1>, (const void*)&v);
        visit(f.count, &append_obj_line<2>, (const void*)&f);
    }
};
}  // namespace
template <typename Visit>
void each_ply_section(const me_ply::PackArgs& a, Visit&& visit) {
    visit(a.nverts, &append_ply_vertex, (const void*)&a);
    visit(a.nfaces, &append_ply_face, (const void*)&a);
}

// A .glb mesh (glb_format.h), one thread.  The formats a mesh destination's suffix selects:
enum MeshFormat { kFormatObj = 0, kFormatPly = 1, kFormatGlb = 2 };

// what stands between positions and indices: colours follow the colour array, as the PLY records do; UVs the mode
inline int glb_second(bool texture_mode, bool with_color) {
    return texture_mode ? me_glb::kUvs : with_color ? me_glb::kColors : me_glb::kNone;
}

// The file's size checked against the u32 of its header: "" when it fits.
inline std::string glb_size_error(const me_glb::Layout& l, int64_t json_bytes) {
    const int64_t bytes = me_glb::file_bytes(l, json_bytes);
    return bytes < me_glb::kMaxFileBytes ? std::string() : "a .glb file of " + std::to_string(bytes) + " bytes cannot state its length";
}
inline const char* glb_bounds_error() { return "a .glb file cannot hold a position bound that is not finite"; }

// The whole file on the host: the bounds, the JSON and BIN unit by unit, by the routines the kernels run.  Returns ""
// and fills `file`, or the reason the mesh is refused (nothing written).  The arrays may be null where their count is 0.
inline std::string glb_file_on_host(const float* xyz, const float* uv, const uint8_t* rgb, const int32_t* faces, int64_t nverts,
                                    int64_t nfaces, bool texture_mode, const char* source_path, std::string& file) {
    const me_glb::Layout l = me_glb::layout_of(nverts, nverts ? nfaces : 0, glb_second(texture_mode, rgb != nullptr));
    int32_t bounds[6];
    me_glb::bounds_identity(bounds);
    for (int64_t i = 0; i < nverts; ++i) me_glb::bounds_add_vertex(xyz, i, bounds);
    if (nverts && !me_glb::bounds_finite(bounds)) return glb_bounds_error();
    const std::string json = me_glb::json_text(l, texture_mode, source_path, bounds);
    const std::string size_error = glb_size_error(l, (int64_t)json.size());
    if (!size_error.empty()) return size_error;
    file = me_glb::front_text(l, json);
    if (nverts == 0) return "";
    const size_t front = file.size();
    file.resize(front + (size_t)l.bin_bytes + 16);   // 16 bytes of slack so that BIN can be moved to an aligned address
    // the units are aligned 16-byte stores: pack at the first 16-byte aligned address at or behind BIN's place, move down
    uint8_t* const at = (uint8_t*)&file[front];
    uint8_t* const bin = at + ((16 - ((uintptr_t)at & 15)) & 15);
    const me_glb::PackArgs a = {xyz, uv, rgb, faces, l, bin};
    for (int64_t u = 0; u < me_glb::total_units(l); ++u) me_glb::pack_unit(a, u);
    memmove(at, bin, (size_t)l.bin_bytes);
    file.resize(front + (size_t)l.bin_bytes);
    return "";
}

}  // namespace me_mesh_host
