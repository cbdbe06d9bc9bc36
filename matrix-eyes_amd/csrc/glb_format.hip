// The BIN chunk of a glTF binary (.glb) mesh produced on the GPU: the positions (x, -y, -z as little-endian f32), the
// vertex colours (r, g, b, 255) or the texture coordinates, and the indices, each section at a multiple of 16 bytes
// (glb_format.h has the layout and the per-unit routine).  Two launches per file:
//   glb_bounds_kernel  the exact minima and maxima of the written positions, which the JSON's position accessor must
//                      state: per lane over 16-byte loads, across the wave by shuffles, across the workgroup's four
//                      waves in LDS, across workgroups by one integer atomic min / max per value.  The values are
//                      compared as sign keys (a total order), so every order of combination gives the same bits.
//   glb_pack_kernel    one thread per 16-byte unit of BIN, one aligned 16-byte store each; no LDS staging (the PLY
//                      records need it, their sizes divide nothing), gaps and tail zeroed by the unit that holds them.
// Both are grid-stride loops over a grid sized by what is resident (launch.h).
#include "model.h"
#include "launch.h"
#include "glb_format.h"

namespace me {

namespace {

using namespace me_glb;

__device__ __forceinline__ int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

__global__ __launch_bounds__(kThreads) void glb_bounds_kernel(const float* xyz, int64_t nverts, int32_t* bounds) {
    const int64_t words = 3 * nverts, units = units_of(4 * words);
    int32_t key[6];   // minima and maxima of x, -y, -z: indexed by constants only, so they stay in registers
    bounds_identity(key);
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < units; q += (int64_t)gridDim.x * kThreads) {
        uint32_t w[4];
        load_words(xyz, q, words, w);
        int32_t lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool valid = 4 * q + k < words;
            const int32_t v = sign_key(w[k] ^ flip_mask(q, k));
            lo[k] = valid ? v : kKeyMax, hi[k] = valid ? v : kKeyMin;
        }
        // elements 0 and 3 are component r = q % 3, element 1 is component r + 1, element 2 component r + 2 (mod 3)
        const int r = (int)(q % 3);
        const int32_t alo = imin(lo[0], lo[3]), ahi = imax(hi[0], hi[3]);
        key[0] = imin(key[0], r == 0 ? alo : r == 1 ? lo[2] : lo[1]);
        key[1] = imin(key[1], r == 0 ? lo[1] : r == 1 ? alo : lo[2]);
        key[2] = imin(key[2], r == 0 ? lo[2] : r == 1 ? lo[1] : alo);
        key[3] = imax(key[3], r == 0 ? ahi : r == 1 ? hi[2] : hi[1]);
        key[4] = imax(key[4], r == 0 ? hi[1] : r == 1 ? ahi : hi[2]);
        key[5] = imax(key[5], r == 0 ? hi[2] : r == 1 ? hi[1] : ahi);
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int32_t other = __shfl_xor(key[c], d, 64);
            key[c] = c < 3 ? imin(key[c], other) : imax(key[c], other);
        }
    }
    __shared__ int32_t part[kThreads / 64][6];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) part[wave][c] = key[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = (int)threadIdx.x;
        int32_t v = part[0][c];
        for (int wv = 1; wv < kThreads / 64; ++wv) v = c < 3 ? imin(v, part[wv][c]) : imax(v, part[wv][c]);
        if (c < 3) atomicMin(&bounds[c], v);
        else atomicMax(&bounds[c], v);
    }
}

__global__ __launch_bounds__(kThreads) void glb_pack_kernel(PackArgs a) {
    const int64_t units = total_units(a.l);
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += (int64_t)gridDim.x * kThreads) pack_unit(a, u);
}

}  // namespace

void glb_bounds_run(const float* xyz, int64_t nverts, int32_t* bounds_dev, int32_t keys[6], hipStream_t s) {
    ME_CHECK(nverts > 0 && nverts <= (int64_t)1 << 29, ME_ERR_BAD_ARG, "glb_bounds: %lld vertices", (long long)nverts);
    // the identities of min and max as bit patterns, set on the stream without host memory
    ME_HIP(hipMemsetD32Async((hipDeviceptr_t)bounds_dev, kKeyMax, 3, s));
    ME_HIP(hipMemsetD32Async((hipDeviceptr_t)(bounds_dev + 3), kKeyMin, 3, s));
    static PerDeviceOnce once;
    auto kern = glb_bounds_kernel;
    const int64_t tiles = cdiv(units_of(12 * nverts), (int64_t)kThreads);
    const unsigned grid = persistent_launch_grid(once, (const void*)kern, kThreads, 0, tiles, "glb_bounds");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), 0, s, xyz, nverts, bounds_dev);
    ME_HIP(hipGetLastError());
    ME_HIP(hipMemcpyAsync(keys, bounds_dev, 24, hipMemcpyDeviceToHost, s));
    ME_HIP(hipStreamSynchronize(s));
}

void glb_pack_launch(const float* xyz, const float* uv, const uint8_t* vertex_rgb, const int32_t* faces, int64_t nverts,
                     int64_t nfaces, int second, uint8_t* bin, hipStream_t s) {
    ME_CHECK(nverts > 0 && nfaces >= 0 && second >= kNone && second <= kUvs, ME_ERR_BAD_ARG, "glb_pack: bad argument");
    ME_CHECK(((uintptr_t)bin & 15) == 0 && ((uintptr_t)xyz & 15) == 0 && ((uintptr_t)uv & 15) == 0 && ((uintptr_t)faces & 15) == 0 &&
                 ((uintptr_t)vertex_rgb & 3) == 0,
             ME_ERR_BAD_ARG, "glb_pack: a buffer is not aligned (16 bytes; the colours 4)");
    ME_CHECK((second != kColors || vertex_rgb) && (second != kUvs || uv) && (nfaces == 0 || faces), ME_ERR_BAD_ARG,
             "glb_pack: null pointer");
    const PackArgs a = {xyz, uv, vertex_rgb, faces, layout_of(nverts, nfaces, second), bin};
    ME_CHECK(a.l.bin_bytes < kMaxFileBytes, ME_ERR_BAD_ARG, "glb_pack: %lld bytes", (long long)a.l.bin_bytes);
    static PerDeviceOnce once;
    auto kern = glb_pack_kernel;
    const int64_t tiles = cdiv(total_units(a.l), (int64_t)kThreads);
    const unsigned grid = persistent_launch_grid(once, (const void*)kern, kThreads, 0, tiles, "glb_pack");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), 0, s, a);
    ME_HIP(hipGetLastError());
}

}  // namespace me
