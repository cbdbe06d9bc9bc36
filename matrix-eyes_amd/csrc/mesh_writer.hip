// output.rs:195-261 output_mesh and its two writers (ObjWriter :484-630, PlyWriter :385-482).
// Vertex ids, faces and coordinates come from the GPU kernels in output.hip, the OBJ text from obj_format.hip, the
// PLY records from ply_format.hip and a glTF binary's sections (".glb": not a format of the reference's) from
// glb_format.hip; this file drives them and hands the finished bytes, copied to the host once, to the
// file writer (file_write.hip, write-behind included).  The host-side serialisers (mesh_host_format.h: the same line,
// record and unit text, run on the host) stay as the A/B of each (ME_OBJ_HOST_FORMAT, ME_PLY_HOST_FORMAT, ME_GLB_HOST_FORMAT).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "model.h"
#include "mesh_host_format.h"

using namespace me;
using namespace me_mesh_host;

namespace {

// what the three mesh entries are asked for
struct MeshRequest {
    const float* depth;
    int32_t width, height;
    uint32_t original_width, original_height;
    int32_t vertex_mode;
    const uint8_t* vertex_colors;
    bool with_color() const { return vertex_mode == ME_VERTEX_COLOR && vertex_colors; }
    size_t pixels() const { return (size_t)width * height; }
};

void check_mesh_args(const char* who, bool pointers, const MeshRequest& r) {
    ME_CHECK(pointers, ME_ERR_BAD_ARG, "%s: null pointer", who);
    ME_CHECK(r.vertex_mode >= ME_VERTEX_PLAIN && r.vertex_mode <= ME_VERTEX_TEXTURE, ME_ERR_BAD_ARG, "vertex mode %d",
             r.vertex_mode);
    ME_CHECK(r.width >= 2 && r.height >= 2, ME_ERR_BAD_SHAPE, "%s: %dx%d", who, r.width, r.height);
    ME_CHECK(r.original_width > 0 && r.original_height > 0, ME_ERR_BAD_ARG, "original size 0");
}

// output.rs:222-225: original / max(original), an f32 division of the u32 sizes
struct SizeRatio {
    float xm, ym;
    SizeRatio(uint32_t original_width, uint32_t original_height) {
        const uint32_t mx = original_width > original_height ? original_width : original_height;
        xm = (float)original_width / (float)mx, ym = (float)original_height / (float)mx;
    }
};

// Everything of output.rs:195-261 that is arithmetic, on the device: IndexedMesh::new + remap_face, the vertex
// coordinates, and the file's bytes themselves.
struct DeviceMesh {
    int64_t nverts = 0, nfaces = 0;
    int32_t* vindex = nullptr;
    int32_t* faces = nullptr;
    float *uv = nullptr, *xyz = nullptr;
};

DeviceMesh build_mesh(me_ctx* ctx, const MeshRequest& r) {
    DeviceMesh m;
    const size_t nv = r.pixels();
    const size_t nt = 2 * (size_t)(r.width - 1) * (r.height - 1);
    const float* d = (const float*)to_device(ctx, r.depth, nv * 4, "out.depth");
    m.vindex = (int32_t*)site_buf(ctx, "out.vindex", nv * 4);
    m.faces = (int32_t*)site_buf(ctx, "out.faces", nt * 12);
    mesh_index_run(d, r.width, r.height, m.vindex, m.faces, &m.nverts, &m.nfaces,
                   site_buf(ctx, "out.mesh.ws", mesh_workspace_bytes(r.width, r.height)), ctx->stream);
    m.uv = (float*)site_buf(ctx, "out.uv", m.nverts * 8 + 8);
    m.xyz = (float*)site_buf(ctx, "out.xyz", m.nverts * 12 + 12);
    const SizeRatio ratio(r.original_width, r.original_height);
    mesh_vertices_launch(d, r.width, r.height, m.vindex, ratio.xm, ratio.ym, m.uv, m.xyz, ctx->stream);
    return m;
}

// colours by vertex id in device memory (the caller's per-pixel array may be on either side), or null when none are written
const uint8_t* vertex_colors_on_device(me_ctx* ctx, const DeviceMesh& m, const MeshRequest& r) {
    if (!r.with_color()) return nullptr;
    const uint8_t* pix = (const uint8_t*)to_device(ctx, r.vertex_colors, r.pixels() * 3, "out.pixel_rgb");
    uint8_t* v = (uint8_t*)site_buf(ctx, "out.vertex_rgb", (size_t)m.nverts * 3 + 16);
    obj_vertex_colors_launch(m.vindex, pix, (int64_t)r.pixels(), v, ctx->stream);
    return v;
}

// the site buffer a file of `bytes` is made in: its size follows the kept faces of each image
char* file_site_buf(me_ctx* ctx, const char* name, int64_t bytes) { return (char*)site_buf(ctx, name, grow_in_steps((size_t)bytes + 64)); }

// The OBJ text in device memory (site buffer "out.objtext"): header lines + vt / v / f sections.
DeviceFile obj_text_on_device(me_ctx* ctx, const DeviceMesh& m, const MeshRequest& r, const std::string& stem) {
    const bool tex = r.vertex_mode == ME_VERTEX_TEXTURE;
    const uint8_t* vrgb = vertex_colors_on_device(ctx, m, r);
    const std::string header = tex ? obj_header(stem) : std::string();
    void* ws = site_buf(ctx, "out.objfmt.ws", obj_format_workspace_bytes(m.nverts, m.nfaces));
    const int64_t bytes = obj_format_measure(m.uv, m.xyz, vrgb, m.faces, m.nverts, m.nfaces, tex, (int64_t)header.size(), ws,
                                             ctx->stream);
    char* text = file_site_buf(ctx, "out.objtext", bytes);
    if (!header.empty()) ME_HIP(hipMemcpyAsync(text, header.data(), header.size(), hipMemcpyHostToDevice, ctx->stream));
    obj_format_write(m.uv, m.xyz, vrgb, m.faces, m.nverts, m.nfaces, tex, text, ws, ctx->stream);
    return {(const uint8_t*)text, bytes};
}

// The PLY file in device memory (site buffer "out.plybytes"): the header, copied in, + the records ply_format.hip packs
// behind it.  The size is closed-form, so nothing comes back to the host in between.
DeviceFile ply_bytes_on_device(me_ctx* ctx, const DeviceMesh& m, const MeshRequest& r) {
    const uint8_t* vrgb = vertex_colors_on_device(ctx, m, r);
    const std::string header = ply_header(m.nverts, m.nfaces, r.vertex_mode == ME_VERTEX_COLOR);
    const int64_t bytes = ply_pack_bytes(m.nverts, vrgb != nullptr, m.nfaces, (int64_t)header.size());
    char* file = file_site_buf(ctx, "out.plybytes", bytes);
    ME_HIP(hipMemcpyAsync(file, header.data(), header.size(), hipMemcpyHostToDevice, ctx->stream));
    ply_pack_launch(m.xyz, vrgb, m.nverts, m.faces, m.nfaces, (int64_t)header.size(), (uint8_t*)file, ctx->stream);
    return {(const uint8_t*)file, bytes};
}

// The .glb file in device memory (site buffer "out.glbbytes"): the bounds of the written positions come back to the host
// (24 bytes, right behind the counts build_mesh read back), the host builds the JSON around them and copies it in with
// the chunk headers, and one launch packs every section of BIN behind it.  An empty mesh is the JSON chunk alone.
DeviceFile glb_bytes_on_device(me_ctx* ctx, const DeviceMesh& m, const MeshRequest& r, const char* source_path) {
    const bool tex = r.vertex_mode == ME_VERTEX_TEXTURE;
    const me_glb::Layout l = me_glb::layout_of(m.nverts, m.nverts ? m.nfaces : 0, glb_second(tex, r.with_color()));
    int32_t bounds[6];
    me_glb::bounds_identity(bounds);
    if (m.nverts) {
        glb_bounds_run(m.xyz, m.nverts, (int32_t*)site_buf(ctx, "out.glb.bounds", 32), bounds, ctx->stream);
        ME_CHECK(me_glb::bounds_finite(bounds), ME_ERR_BAD_ARG, "%s", glb_bounds_error());
    }
    const std::string json = me_glb::json_text(l, tex, source_path, bounds);
    const std::string size_error = glb_size_error(l, (int64_t)json.size());
    ME_CHECK(size_error.empty(), ME_ERR_BAD_ARG, "%s", size_error.c_str());
    const std::string front = me_glb::front_text(l, json);
    const int64_t bytes = me_glb::file_bytes(l, (int64_t)json.size());
    char* file = file_site_buf(ctx, "out.glbbytes", bytes);
    ME_HIP(hipMemcpyAsync(file, front.data(), front.size(), hipMemcpyHostToDevice, ctx->stream));
    if (m.nverts) {
        const uint8_t* vrgb = vertex_colors_on_device(ctx, m, r);
        glb_pack_launch(m.xyz, m.uv, vrgb, m.faces, m.nverts, m.nfaces, l.second, (uint8_t*)file + front.size(), ctx->stream);
    }
    return {(const uint8_t*)file, bytes};
}

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// The file's bytes are produced on the GPU too (OBJ: the text, obj_format.hip; PLY: the binary records, ply_format.hip;
// GLB: the BIN sections, glb_format.hip, behind the JSON the host builds from the bounds the GPU reduced);
// one D2H copy into pinned memory, one file write.  With write-behind this call's bytes go into the pinned buffer whose
// earlier write has finished (waited for here, a failure of it reported here), and a host thread writes the file while
// the caller moves on.
void write_device_mesh(me_ctx* ctx, const DeviceMesh& mesh, const MeshRequest& r, const std::string& dest, MeshFormat format,
                       const char* source_path, Clock::time_point t_entry) {
    const bool obj = format == kFormatObj;
    static const bool timing = getenv("ME_OBJ_TIMING") != nullptr;  // diagnostic: the legs on stderr
    const auto t0 = Clock::now();
    const DeviceFile t = obj                    ? obj_text_on_device(ctx, mesh, r, file_stem(dest))
                         : format == kFormatPly ? ply_bytes_on_device(ctx, mesh, r)
                                                : glb_bytes_on_device(ctx, mesh, r, source_path);
    PinnedFile file;
    file.dest = dest, file.bytes = (size_t)t.bytes, file.slot = ctx->write_behind ? ctx->write_next : 0;
    if (obj && r.vertex_mode == ME_VERTEX_TEXTURE) file.side_path = mtl_path(dest), file.side_text = mtl_text(source_path);
    if (ctx->write_behind) join_pending_write(ctx, file.slot);
    char* host = pinned_buf(ctx, file.bytes, file.slot);
    file.data = host;
    ME_HIP(hipStreamSynchronize(ctx->stream));  // the legs are reported separately (me_last_mesh_timing)
    const auto t1 = Clock::now();
    ME_HIP(hipMemcpyAsync(host, t.dev, file.bytes, hipMemcpyDeviceToHost, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    const auto t2 = Clock::now();
    write_pinned_file(ctx, file, ctx->write_behind != 0);
    if (ctx->write_behind) ctx->write_next = (ctx->write_next + 1) % ctx->write_behind;
    const auto t3 = Clock::now();
    const double ms[4] = {ms_between(t_entry, t0), ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, t3)};
    memcpy(ctx->mesh_ms, ms, sizeof ms);
    ctx->mesh_bytes = t.bytes;
    if (timing)
        fprintf(stderr, "me_output_mesh: %lld vertices, %lld faces, %lld bytes: mesh %.2f ms, format %.2f ms, D2H %.2f ms, "
                        "file %.2f ms\n", (long long)mesh.nverts, (long long)mesh.nfaces, (long long)t.bytes, ms[0], ms[1], ms[2], ms[3]);
}

// colours by vertex id on the host: the pixel that first used a vertex gives it its colour (output.rs:206-218, 578-587)
std::vector<uint8_t> host_vertex_colors(me_ctx* ctx, const DeviceMesh& mesh, const MeshRequest& r) {
    const size_t nv = r.pixels();
    std::vector<int32_t> vi(nv);
    ME_HIP(hipMemcpyAsync(vi.data(), mesh.vindex, nv * 4, hipMemcpyDeviceToHost, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<uint8_t> host_colors;
    const uint8_t* src = r.vertex_colors;
    if (is_device_ptr(r.vertex_colors)) {
        host_colors.resize(nv * 3);
        ME_HIP(hipMemcpy(host_colors.data(), r.vertex_colors, nv * 3, hipMemcpyDeviceToHost));
        src = host_colors.data();
    }
    std::vector<uint8_t> colors((size_t)mesh.nverts * 3);
    for (size_t i = 0; i < nv; ++i)
        if (vi[i] >= 0) memcpy(&colors[(size_t)vi[i] * 3], src + i * 3, 3);
    return colors;
}

// ME_OBJ_HOST_FORMAT=1 / ME_PLY_HOST_FORMAT=1 / ME_GLB_HOST_FORMAT=1: the mesh comes back to the host and
// mesh_host_format.h serialises it (the same bytes; the A/B of each device formatter).  OBJ sections are formatted by up
// to 12 threads; a PLY record is a byte shuffle per item, not worth the second copy; a GLB is made whole by one thread.
void write_host_mesh(me_ctx* ctx, const DeviceMesh& mesh, const MeshRequest& r, const std::string& dest, MeshFormat format,
                     const char* source_path) {
    const bool obj = format == kFormatObj;
    const int64_t nverts = mesh.nverts, nfaces = mesh.nfaces;
    std::vector<float> uv((size_t)nverts * 2), xyz((size_t)nverts * 3);
    std::vector<int32_t> faces((size_t)nfaces * 3);
    if (nverts) {
        ME_HIP(hipMemcpyAsync(uv.data(), mesh.uv, uv.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        ME_HIP(hipMemcpyAsync(xyz.data(), mesh.xyz, xyz.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (nfaces) ME_HIP(hipMemcpyAsync(faces.data(), mesh.faces, faces.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<uint8_t> colors;  // per vertex id
    if (r.with_color()) colors = host_vertex_colors(ctx, mesh, r);
    const uint8_t* rgb = r.with_color() ? colors.data() : nullptr;

    std::vector<FileSection> sections;
    const auto add = [&](bool threads) {
        return [&sections, threads](int64_t count, AppendItem item, const void* args) { sections.push_back({count, item, args, threads}); };
    };
    if (format == kFormatGlb) {
        std::string file;
        const std::string refused = glb_file_on_host(xyz.data(), uv.data(), rgb, faces.data(), nverts, nfaces,
                                                     r.vertex_mode == ME_VERTEX_TEXTURE, source_path, file);
        ME_CHECK(refused.empty(), ME_ERR_BAD_ARG, "%s", refused.c_str());
        write_sections(dest, file, nullptr, 0);
    } else if (obj) {
        const bool tex = r.vertex_mode == ME_VERTEX_TEXTURE;
        const ObjSections text(uv.data(), xyz.data(), rgb, faces.data(), nverts, nfaces, tex);
        text.each(add(true));
        write_sections(dest, tex ? obj_header(file_stem(dest)) : std::string(), sections.data(), (int)sections.size());
        if (tex) write_sections(mtl_path(dest), mtl_text(source_path), nullptr, 0);
    } else {
        const me_ply::PackArgs records = {xyz.data(), rgb, faces.data(), nverts, nfaces, 0, nullptr};
        each_ply_section(records, add(false));
        write_sections(dest, ply_header(nverts, nfaces, r.vertex_mode == ME_VERTEX_COLOR), sections.data(), (int)sections.size());
    }
}

}  // namespace

extern "C" int32_t me_last_mesh_timing(const me_ctx* ctx, double ms_out[4], int64_t* text_bytes) {
    if (!ctx || !ms_out) return ME_ERR_BAD_ARG;
    for (int i = 0; i < 4; ++i) ms_out[i] = ctx->mesh_ms[i];
    if (text_bytes) *text_bytes = ctx->mesh_bytes;
    return ME_OK;
}

extern "C" int32_t me_mesh_index(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                                 int32_t* vertex_index, int64_t* nvertices, int64_t* nfaces, int32_t* faces) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && vertex_index && nvertices && nfaces, ME_ERR_BAD_ARG,
             "me_mesh_index: null pointer");
    ME_CHECK(width >= 2 && height >= 2, ME_ERR_BAD_SHAPE, "me_mesh_index: %dx%d", width, height);
    const size_t nv = (size_t)width * height;
    const size_t nt = 2 * (size_t)(width - 1) * (height - 1);
    const float* d = (const float*)to_device(ctx, depth, nv * 4, "out.depth");
    OutBuf ov = out_buf(ctx, vertex_index, nv * 4, "out.vindex");
    OutBuf of;
    if (faces) of = out_buf(ctx, faces, nt * 3 * 4, "out.faces");
    mesh_index_run(d, width, height, (int32_t*)ov.dev, faces ? (int32_t*)of.dev : nullptr, nvertices,
                   nfaces, site_buf(ctx, "out.mesh.ws", mesh_workspace_bytes(width, height)), ctx->stream);
    finish(ctx, ov);
    if (faces && of.staged) {  // only the kept triangles are defined
        ME_HIP(hipMemcpyAsync(faces, of.dev, (size_t)*nfaces * 12, hipMemcpyDeviceToHost,
                              ctx->stream));
        ME_HIP(hipStreamSynchronize(ctx->stream));
    }
    ME_API_END(ctx)
}

extern "C" int32_t me_mesh_vertices(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                                    const int32_t* vertex_index, int64_t nvertices, uint32_t original_width,
                                    uint32_t original_height, float* uv, float* xyz) {
    ME_API_BEGIN(ctx)
    OutputScope out_scope(ctx, depth);
    ME_CHECK(depth && vertex_index && nvertices >= 0, ME_ERR_BAD_ARG, "me_mesh_vertices: bad argument");
    ME_CHECK(original_width > 0 && original_height > 0, ME_ERR_BAD_ARG, "original size 0");
    const size_t nv = (size_t)width * height;
    const float* d = (const float*)to_device(ctx, depth, nv * 4, "out.depth");
    const int32_t* vi = (const int32_t*)to_device(ctx, vertex_index, nv * 4, "out.vindex");
    const SizeRatio ratio(original_width, original_height);
    OutBuf ouv, oxyz;
    if (uv) ouv = out_buf(ctx, uv, (size_t)nvertices * 8 + 8, "out.uv");
    if (xyz) oxyz = out_buf(ctx, xyz, (size_t)nvertices * 12 + 12, "out.xyz");
    mesh_vertices_launch(d, width, height, vi, ratio.xm, ratio.ym, uv ? (float*)ouv.dev : nullptr,
                         xyz ? (float*)oxyz.dev : nullptr, ctx->stream);
    if (uv && ouv.staged) from_device(ctx, uv, ouv.dev, (size_t)nvertices * 8);
    if (xyz && oxyz.staged) from_device(ctx, xyz, oxyz.dev, (size_t)nvertices * 12);
    ME_API_END(ctx)
}

extern "C" int32_t me_mesh_obj_text(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                                    uint32_t original_width, uint32_t original_height, const char* stem,
                                    int32_t vertex_mode, const uint8_t* vertex_colors, const uint8_t** text_dev,
                                    int64_t* nbytes) {
    ME_API_BEGIN(ctx)
    const MeshRequest r = {depth, width, height, original_width, original_height, vertex_mode, vertex_colors};
    check_mesh_args("me_mesh_obj_text", depth && stem && text_dev && nbytes, r);
    OutputScope out_scope(ctx, depth);
    const DeviceFile t = obj_text_on_device(ctx, build_mesh(ctx, r), r, stem);
    ME_HIP(hipStreamSynchronize(ctx->stream));
    *text_dev = t.dev, *nbytes = t.bytes;
    ME_API_END(ctx)
}

extern "C" int32_t me_mesh_ply_bytes(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                                     uint32_t original_width, uint32_t original_height, int32_t vertex_mode,
                                     const uint8_t* vertex_colors, const uint8_t** bytes_dev, int64_t* nbytes) {
    ME_API_BEGIN(ctx)
    const MeshRequest r = {depth, width, height, original_width, original_height, vertex_mode, vertex_colors};
    check_mesh_args("me_mesh_ply_bytes", depth && bytes_dev && nbytes, r);
    OutputScope out_scope(ctx, depth);
    const DeviceFile t = ply_bytes_on_device(ctx, build_mesh(ctx, r), r);
    ME_HIP(hipStreamSynchronize(ctx->stream));
    *bytes_dev = t.dev, *nbytes = t.bytes;
    ME_API_END(ctx)
}

extern "C" int32_t me_mesh_glb_bytes(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                                     uint32_t original_width, uint32_t original_height, const char* source_path,
                                     int32_t vertex_mode, const uint8_t* vertex_colors, const uint8_t** bytes_dev,
                                     int64_t* nbytes) {
    ME_API_BEGIN(ctx)
    const MeshRequest r = {depth, width, height, original_width, original_height, vertex_mode, vertex_colors};
    check_mesh_args("me_mesh_glb_bytes", depth && source_path && bytes_dev && nbytes, r);
    OutputScope out_scope(ctx, depth);
    const DeviceFile t = glb_bytes_on_device(ctx, build_mesh(ctx, r), r, source_path);
    ME_HIP(hipStreamSynchronize(ctx->stream));
    *bytes_dev = t.dev, *nbytes = t.bytes;
    ME_API_END(ctx)
}

// Its own catch block: an exception that is not an me::Error is an I/O failure here (ME_ERR_IO, not ME_API_END's ME_ERR_BAD_ARG)
extern "C" int32_t me_output_mesh(me_ctx* ctx, const float* depth, int32_t width, int32_t height,
                                  uint32_t original_width, uint32_t original_height,
                                  const char* destination_path, const char* source_path,
                                  int32_t vertex_mode, const uint8_t* vertex_colors) {
    if (!ctx) return ME_ERR_BAD_ARG;
    try {
        ME_HIP(hipSetDevice(ctx->device));
        const MeshRequest r = {depth, width, height, original_width, original_height, vertex_mode, vertex_colors};
        check_mesh_args("me_output_mesh", depth && destination_path && source_path, r);
        const std::string dest(destination_path);
        const bool ply = ends_with_ci(dest, ".ply"), obj = ends_with_ci(dest, ".obj"), glb = ends_with_ci(dest, ".glb");
        ME_CHECK(ply || obj || glb, ME_ERR_BAD_ARG, "mesh destination must end in .obj, .ply or .glb: %s", destination_path);
        const MeshFormat format = obj ? kFormatObj : ply ? kFormatPly : kFormatGlb;
        OutputScope out_scope(ctx, depth);
        const auto t_entry = Clock::now();
        if (ctx->write_behind) {
            // Before any GPU work of this call: the pinned buffer it will use must be free, and a failed earlier write
            // is reported NOW (this call has produced nothing yet; the caller can repeat it).  A pending write to the
            // same destination is waited for as well -- a second fopen("wb") would truncate the file under it.
            join_pending_write(ctx, ctx->write_next);
            for (int k = 0; k < (int)ctx->write_slots.size(); ++k)
                if (ctx->write_slots[(size_t)k].active && ctx->write_slots[(size_t)k].dest == dest) join_pending_write(ctx, k);
        }
        const DeviceMesh mesh = build_mesh(ctx, r);
        static const bool obj_host_format = getenv("ME_OBJ_HOST_FORMAT") != nullptr;
        static const bool ply_host_format = getenv("ME_PLY_HOST_FORMAT") != nullptr;
        static const bool glb_host_format = getenv("ME_GLB_HOST_FORMAT") != nullptr;
        if (obj ? obj_host_format : ply ? ply_host_format : glb_host_format) write_host_mesh(ctx, mesh, r, dest, format, source_path);
        else write_device_mesh(ctx, mesh, r, dest, format, source_path, t_entry);
    } catch (const me::Error& e) {
        ctx->last_error = e.msg;
        return e.code;
    } catch (const std::exception& e) {
        ctx->last_error = std::string("internal: ") + e.what();
        return ME_ERR_IO;
    }
    return ME_OK;
}
