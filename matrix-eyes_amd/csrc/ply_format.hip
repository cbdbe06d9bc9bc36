// The body of a binary PLY file produced on the GPU (reference src/output.rs:385-482 PlyWriter): the vertex records
// (x, -y, -z as big-endian f64, optionally r g b) and the face records (3 + three big-endian u32) packed back to back
// behind the ASCII header in ONE byte buffer, so that a 1536x1536 mesh (118 - 125 MB) costs one D2H copy and one file
// write instead of a single-threaded byte-at-a-time host loop beside a 22 ms forward pass.
//
// One launch per file: the record sizes are fixed, so every workgroup knows where its records go (ply_format.h
// span_of) -- no measure or scan pass as the OBJ text needs.  A workgroup stages its 256 records in LDS at the
// residue mod 16 of their destination and writes them as aligned 16-byte chunks (ply_format.h pack_block).
#include "model.h"
#include "ply_format.h"

namespace me {

namespace {

__global__ __launch_bounds__(me_ply::kThreads) void ply_pack_kernel(me_ply::PackArgs a, int64_t first_block) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[me_ply::kStageBytes];
    me_ply::pack_block(a, first_block + blockIdx.x, stage);
}

}  // namespace

int64_t ply_pack_bytes(int64_t nverts, bool with_rgb, int64_t nfaces, int64_t header_bytes) {
    return header_bytes + nverts * (me_ply::kVertexBytes + (with_rgb ? me_ply::kColorBytes : 0)) + nfaces * me_ply::kFaceBytes;
}

void ply_pack_launch(const float* xyz, const uint8_t* vertex_rgb, int64_t nverts, const int32_t* faces, int64_t nfaces,
                     int64_t header_bytes, uint8_t* out, hipStream_t s) {
    ME_CHECK(nverts >= 0 && nfaces >= 0 && header_bytes >= 0, ME_ERR_BAD_ARG, "ply_pack: negative count");
    ME_CHECK(nverts <= (int64_t)INT32_MAX + 1, ME_ERR_BAD_ARG, "ply_pack: %lld vertices (ids are 32-bit)", (long long)nverts);
    const me_ply::PackArgs a = {xyz, vertex_rgb, faces, nverts, nfaces, header_bytes, out};
    const int64_t blocks = me_ply::blocks_of(nverts) + me_ply::blocks_of(nfaces);
    constexpr int64_t kGrid = 1 << 30;   // workgroups per launch
    for (int64_t first = 0; first < blocks; first += kGrid) {
        const int64_t n = blocks - first < kGrid ? blocks - first : kGrid;
        hipLaunchKernelGGL(ply_pack_kernel, dim3((unsigned)n), dim3(me_ply::kThreads), 0, s, a, first);
        ME_HIP(hipGetLastError());
    }
}

}  // namespace me
