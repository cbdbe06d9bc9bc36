// The PLY writer's record and workgroup routines (matrix-eyes_amd/csrc/ply_format.h) run on the host, workgroup by
// workgroup and lane by lane, the way ply_pack_kernel runs them:
//   ply_format_host <cases file> <files file>
// cases file: i64 count, then per case i64 header_bytes, nverts, nfaces, has_rgb; the header's bytes; xyz f32
// [nverts][3]; rgb u8 [nverts][3] if has_rgb; faces i32 [nfaces][3] (native byte order).
// files file: per case i64 nbytes and the file the GPU kernel writes behind that header (tests/test_ply_cpu.py
// compares it with the oracle's).  Exit 3: a byte outside the file was written.
#define ME_PLY_HOST 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../matrix-eyes_amd/csrc/ply_format.h"

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
    using namespace me_ply;
    constexpr size_t kGuard = 64;
    for (int64_t k = 0; k < ncases; ++k) {
        int64_t head[4];
        if (!get(in, head, 4) || head[0] < 0 || head[1] < 0 || head[2] < 0) return 1;
        const int64_t header_bytes = head[0], nverts = head[1], nfaces = head[2];
        // exactly sized, so that a read past an array's end is a sanitizer report
        std::vector<uint8_t> header((size_t)header_bytes), rgb(head[3] ? (size_t)nverts * 3 : 0);
        std::vector<float> xyz((size_t)nverts * 3);
        std::vector<int32_t> faces((size_t)nfaces * 3);
        if (!get(in, header.data(), header.size()) || !get(in, xyz.data(), xyz.size()) || !get(in, rgb.data(), rgb.size()) ||
            !get(in, faces.data(), faces.size()))
            return 1;
        PackArgs a = {xyz.data(), head[3] ? rgb.data() : nullptr, faces.data(), nverts, nfaces, header_bytes, nullptr};
        const int64_t nbytes = file_bytes(a);
        // 16-byte aligned like the device buffer: the residue of a span's address is the residue of its place in the file
        void* mem = nullptr;
        if (posix_memalign(&mem, 16, (size_t)nbytes + kGuard) != 0) return 1;
        a.out = (uint8_t*)mem;
        memset(a.out, 0xEE, (size_t)nbytes + kGuard);
        memcpy(a.out, header.data(), header.size());   // the caller's H2D copy
        alignas(16) uint8_t stage[kStageBytes];
        const int64_t blocks = blocks_of(nverts) + blocks_of(nfaces);
        for (int64_t b = 0; b < blocks; ++b) {
            memset(stage, (int)(0x11 * (b % 15 + 1)), sizeof stage);   // what another workgroup left in the LDS
            pack_block(a, b, stage);
        }
        for (size_t g = 0; g < kGuard; ++g)
            if (a.out[nbytes + (int64_t)g] != 0xEE) {
                fprintf(stderr, "case %lld: byte %zu behind the file was written\n", (long long)k, g);
                return 3;
            }
        if (memcmp(a.out, header.data(), header.size()) != 0) {
            fprintf(stderr, "case %lld: the header was written over\n", (long long)k);
            return 3;
        }
        if (fwrite(&nbytes, 8, 1, out) != 1 || (nbytes && fwrite(a.out, 1, (size_t)nbytes, out) != (size_t)nbytes)) return 1;
        free(mem);
    }
    fclose(in);
    if (fclose(out) != 0) return 1;
    return 0;
}
