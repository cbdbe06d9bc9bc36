// The .glb writer's layout, JSON builder and per-unit routines (matrix-eyes_amd/csrc/glb_format.h in host mode) and the
// one-thread host serialiser made of them (mesh_host_format.h glb_file_on_host, what ME_GLB_HOST_FORMAT=1 runs):
//   glb_format_host <cases file> <files file>
// cases file: i64 count, then per case i64 mode (0 plain, 1 colour, 2 texture), nverts, nfaces, has_rgb, source_bytes;
// the source path's bytes; uv f32 [nverts][2]; xyz f32 [nverts][3]; rgb u8 [nverts][3] if has_rgb; faces i32 [nfaces][3].
// files file: per case i64 refused (0 / 1), i64 nbytes and the file (tests/test_glb_cpu.py compares it with its own
// restatement).  Besides the serialiser's file, BIN is packed unit by unit -- the loop of glb_pack_kernel -- into a
// heap block of exactly its size, so that the sanitizer sees a byte written beside it; exit 3 when the two differ.
#define ME_OBJ_HOST 1
#define ME_PLY_HOST 1
#define ME_GLB_HOST 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../matrix-eyes_amd/csrc/mesh_host_format.h"

namespace {

template <class T>
bool get(FILE* f, T* p, size_t n) {
    return n == 0 || fread(p, sizeof(T), n, f) == n;
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
        int64_t head[5];
        if (!get(in, head, 5) || head[0] < 0 || head[0] > 2 || head[1] < 0 || head[2] < 0 || head[4] < 0) return 1;
        const bool texture = head[0] == 2;
        const int64_t nverts = head[1], nfaces = head[2];
        // exactly sized, so that a read past an array's end is a sanitizer report
        std::string source((size_t)head[4], '\0');
        std::vector<float> uv((size_t)nverts * 2), xyz((size_t)nverts * 3);
        std::vector<uint8_t> rgb(head[3] ? (size_t)nverts * 3 : 0);
        std::vector<int32_t> faces((size_t)nfaces * 3);
        if (!get(in, &source[0], source.size()) || !get(in, uv.data(), uv.size()) || !get(in, xyz.data(), xyz.size()) ||
            !get(in, rgb.data(), rgb.size()) || !get(in, faces.data(), faces.size()))
            return 1;
        const uint8_t* colors = head[3] && head[0] == 1 ? rgb.data() : nullptr;   // read in colour mode only
        std::string file;
        const std::string refused = me_mesh_host::glb_file_on_host(xyz.data(), uv.data(), colors, faces.data(), nverts, nfaces,
                                                                   texture, source.c_str(), file);
        const int64_t flag = refused.empty() ? 0 : 1, nbytes = refused.empty() ? (int64_t)file.size() : 0;
        if (refused.empty() && nverts) {
            using namespace me_glb;
            const Layout l = layout_of(nverts, nfaces, me_mesh_host::glb_second(texture, colors != nullptr));
            if ((int64_t)file.size() < l.bin_bytes || (file.size() - (size_t)l.bin_bytes) % 16 != 0) {
                fprintf(stderr, "case %lld: BIN does not start at a multiple of 16\n", (long long)k);
                return 3;
            }
            void* mem = nullptr;
            if (posix_memalign(&mem, 16, (size_t)l.bin_bytes) != 0) return 1;
            memset(mem, 0xEE, (size_t)l.bin_bytes);
            const PackArgs a = {xyz.data(), uv.data(), colors, faces.data(), l, (uint8_t*)mem};
            for (int64_t u = total_units(l) - 1; u >= 0; --u) pack_unit(a, u);   // any order: the units are independent
            const bool same = memcmp(mem, file.data() + file.size() - (size_t)l.bin_bytes, (size_t)l.bin_bytes) == 0;
            free(mem);
            if (!same) {
                fprintf(stderr, "case %lld: the units packed on their own differ from the file's BIN\n", (long long)k);
                return 3;
            }
        }
        if (fwrite(&flag, 8, 1, out) != 1 || fwrite(&nbytes, 8, 1, out) != 1 ||
            (nbytes && fwrite(file.data(), 1, (size_t)nbytes, out) != (size_t)nbytes))
            return 1;
    }
    fclose(in);
    if (fclose(out) != 0) return 1;
    return 0;
}
