// The keyed noise of the stereogram on the device (chacha.h holds the definition and the host twin): the
// fill kernel that writes the [out_h, out_w, 3] picture of noise, and the keyed stereogram, which is that fill into the
// context's scratch followed by stereogram_kernel (output.hip).  A kernel that made each row's words inside the
// stereogram kernel was built, measured against these two launches and deleted: it did not beat them by more than their
// own spread (profiles/stereogram_noise_ab.txt).  Integer work and LDS traffic; the kernel waits on no other workgroup
// and its loops are bounded by the fixed round count.
#include "chacha.h"
#include "model.h"

namespace me {

namespace {

using me_chacha::Key;

// One ChaCha12 block (16 pixels, 48 bytes) per lane, the state in registers.  A wave's 64 blocks are 3072 contiguous
// bytes of the picture: each lane packs its 48 bytes into 12 dwords of the wave's LDS stage, and the wave stores the stage
// as 12 rows of 64 consecutive dwords (256-byte rows) instead of 64 pieces of 48 bytes.  The picture starts at block 0, so
// only its end can cut a block: the last wave stores the whole dwords that lie inside the picture and then the 1 - 3
// bytes behind them.  A destination that is not 4-byte aligned (a caller's slice) takes byte stores throughout.
__global__ __launch_bounds__(256) void stereogram_noise_fill_kernel(Key key, int64_t pixels, uint8_t* __restrict__ out) {
    __shared__ uint32_t stage[4][768];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wave_block0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
    const int64_t b = wave_block0 + lane;
    uint32_t* st = stage[wave];
    if (b * 16 < pixels) {
        uint32_t w[16];
        me_chacha::block<me_chacha::kNoiseRounds>(key, (uint64_t)b, w);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint32_t d[3];
            me_chacha::pack_rgb4(w + 4 * g, d);
            st[lane * 12 + 3 * g + 0] = d[0], st[lane * 12 + 3 * g + 1] = d[1], st[lane * 12 + 3 * g + 2] = d[2];
        }
    }
    __syncthreads();
    const int64_t nbytes = pixels * 3, byte0 = wave_block0 * 48;
    if (byte0 >= nbytes) return;
    const int avail = (int)(nbytes - byte0 < 3072 ? nbytes - byte0 : 3072);  // of this wave's 3072 bytes, inside the picture
    uint8_t* dst = out + byte0;
    if (((size_t)out & 3) == 0) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);  // byte0 is a multiple of 3072
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            const int j = r * 64 + lane;
            if (4 * j + 4 <= avail) d32[j] = st[j];
        }
        const int o = (avail & ~3) + lane;
        if (o < avail) dst[o] = (uint8_t)(st[o >> 2] >> (8 * (o & 3)));
    } else {
        for (int o = lane; o < avail; o += 64) dst[o] = (uint8_t)(st[o >> 2] >> (8 * (o & 3)));
    }
}

}  // namespace

void stereogram_noise_fill_launch(me_ctx* ctx, const uint8_t key[32], int32_t out_w, int32_t out_h, uint8_t* out_dev,
                                  int32_t path) {
    const int64_t pixels = (int64_t)out_w * out_h;
    const int64_t blocks = cdiv(pixels, 16);
    ctx->stereo_noise_marks.record(0, ctx->stream);
    hipLaunchKernelGGL(stereogram_noise_fill_kernel, dim3((unsigned)cdiv(blocks, 256)), dim3(256), 0, ctx->stream,
                       me_chacha::key_from_bytes(key), pixels, out_dev);
    ME_HIP(hipGetLastError());
    ctx->stereo_noise_marks.record(1, ctx->stream);
    ctx->stereo_noise_path = path, ctx->stereo_noise_words = blocks * 16;
}

void stereogram_keyed_launch(me_ctx* ctx, const float* depth_dev, int32_t rows, int32_t cols, float min_depth, float max_depth,
                             const float* range_dev, int32_t out_w, int32_t out_h, float amplitude, const uint8_t key[32],
                             uint8_t* out_dev) {
    stereogram_check_shape(rows, cols, out_w, out_h);  // before the fill: a refused call launches nothing
    uint8_t* noise = (uint8_t*)site_buf(ctx, "out.noise", (size_t)out_w * out_h * 3);
    stereogram_noise_fill_launch(ctx, key, out_w, out_h, noise, 2);
    stereogram_launch(depth_dev, rows, cols, min_depth, max_depth, range_dev, out_w, out_h, amplitude, noise, out_dev, ctx->stream);
}

void free_stereogram_noise_scratch(me_ctx* ctx) { ctx->stereo_noise_marks.destroy(); }

}  // namespace me
