// The host serialisers of the mesh files (matrix-eyes_amd/csrc/mesh_host_format.h over obj_format.h and ply_format.h)
// without a GPU:
//   mesh_format_host <cases file> <files file>
// cases file: i64 count, then per case i64 mode (0 plain, 1 colour, 2 texture), nverts, nfaces, has_rgb, exact_slots,
// dest_bytes, source_bytes; the destination path (".obj" / ".ply", any case) and the source path; uv f32 [nverts][2];
// xyz f32 [nverts][3]; rgb u8 [nverts][3] if has_rgb; faces i32 [nfaces][3] (native byte order).
// files file: per case three blobs, each i64 nbytes + bytes: the file write_host_mesh writes (the sections in
// ObjSections / each_ply_section order behind the header), the path of the .mtl and its text (both empty unless the case
// is a textured OBJ).  tests/test_mesh_format_cpu.py compares them with the oracle's.
// exact_slots (OBJ): every line is formatted by format_line into a heap buffer of exactly the section's slot size
// (kSlotVt / kSlotV / kSlotF, the LDS bytes a thread of obj_lines_kernel has for it), so that the address sanitizer sees
// an overrun.  Exit 3: a line longer than its slot.
#define ME_OBJ_HOST 1
#define ME_PLY_HOST 1
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../matrix-eyes_amd/csrc/mesh_host_format.h"

namespace {

using namespace me_mesh_host;

template <class T>
bool get(FILE* f, T* p, size_t n) {
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}
bool put(FILE* f, const std::string& s) {
    const int64_t n = (int64_t)s.size();
    return fwrite(&n, 8, 1, f) == 1 && (n == 0 || fwrite(s.data(), 1, s.size(), f) == s.size());
}

template <int SEC, int SLOT>
bool exact_lines(const me::ObjArgs& a, std::string& out) {
    for (int64_t i = 0; i < a.count; ++i) {
        std::unique_ptr<char[]> slot(new char[SLOT]);
        const int n = me::format_line<SEC>(a, i, slot.get());
        if (n > SLOT) return false;
        out.append(slot.get(), (size_t)n);
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s cases files\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    int64_t ncases = 0;
    if (!in || !out || !get(in, &ncases, 1)) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 1;
    }
    for (int64_t k = 0; k < ncases; ++k) {
        int64_t head[7];
        if (!get(in, head, 7)) return 1;
        for (int64_t h : head)
            if (h < 0) return 1;
        const int64_t mode = head[0], nverts = head[1], nfaces = head[2];
        const bool exact = head[4] != 0;
        // exactly sized, so that a read past an array's end is a sanitizer report
        std::string dest((size_t)head[5], ' '), source((size_t)head[6], ' ');
        std::vector<float> uv((size_t)nverts * 2), xyz((size_t)nverts * 3);
        std::vector<uint8_t> rgb(head[3] ? (size_t)nverts * 3 : 0);
        std::vector<int32_t> faces((size_t)nfaces * 3);
        if (!get(in, &dest[0], dest.size()) || !get(in, &source[0], source.size()) || !get(in, uv.data(), uv.size()) ||
            !get(in, xyz.data(), xyz.size()) || !get(in, rgb.data(), rgb.size()) || !get(in, faces.data(), faces.size()))
            return 1;
        const bool ply = ends_with_ci(dest, ".ply"), obj = ends_with_ci(dest, ".obj");
        if (ply == obj) return 1;
        const uint8_t* colors = mode == 1 && head[3] ? rgb.data() : nullptr;   // MeshRequest::with_color
        const bool tex = obj && mode == 2;
        const auto all_items = [](std::string& file) {
            return [&file](int64_t count, void (*item)(const void*, int64_t, std::string&), const void* args) {
                for (int64_t i = 0; i < count; ++i) item(args, i, file);
            };
        };
        std::string file;
        if (obj) {
            if (tex) file = obj_header(file_stem(dest));
            const ObjSections text(uv.data(), xyz.data(), colors, faces.data(), nverts, nfaces, tex);
            if (!exact) {
                text.each(all_items(file));
            } else if (!exact_lines<0, me::kSlotVt>(text.vt, file) || !exact_lines<1, me::kSlotV>(text.v, file) ||
                       !exact_lines<2, me::kSlotF>(text.f, file)) {
                fprintf(stderr, "case %lld: a line is longer than its slot\n", (long long)k);
                return 3;
            }
        } else {
            file = ply_header(nverts, nfaces, mode == 1);
            const me_ply::PackArgs records = {xyz.data(), colors, faces.data(), nverts, nfaces, 0, nullptr};
            each_ply_section(records, all_items(file));
        }
        if (!put(out, file) || !put(out, tex ? mtl_path(dest) : std::string()) || !put(out, tex ? mtl_text(source) : std::string()))
            return 1;
    }
    fclose(in);
    if (fclose(out) != 0) return 1;
    return 0;
}
