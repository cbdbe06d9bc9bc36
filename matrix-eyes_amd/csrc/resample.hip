// Lanczos3 resize_exact for 8-bit RGB (reference reconstruction.rs:107-113, output.rs:133-137, output.rs:206-218:
// DynamicImage::resize_exact(nw, nh, FilterType::Lanczos3) of the `image` crate, imageops/sample.rs).
//
// Two passes, as the crate runs them: vertical u8 [h][w][3] -> f32 [nh][w][3] (unclamped), then horizontal f32 ->
// round(clamp(t, 0, 255)) u8 [nh][nw][3].  Per output index the taps [left, left + count) and their normalised
// weights come from a host-built table (lanczos_table.cpp); the kernels only accumulate t += pixel_i * w_i in f32, in
// index order, one channel at a time.
//
// Bit-exactness: every multiply and add is a separately rounded f32 operation (__fmul_rn / __fadd_rn) and the whole
// unit is compiled with contraction off (pragma below and the Makefile rule), as output.hip is: a fused multiply-add
// here changes bytes.  HBM-side kernels, no MFMA.
#include <algorithm>
#include <vector>

#include "lanczos_table.h"
#include "model.h"

#pragma clang fp contract(off)

namespace me {

namespace {

constexpr int kVerticalRows = 4;     // output rows one workgroup of the vertical pass walks, one after the other
constexpr int kLdsFloats = 4096;     // staged span of the horizontal pass: at most 16 KB, so LDS never limits occupancy

// Vertical pass.  A source row is `row_bytes` = 3 * w independent byte columns; a lane owns VEC consecutive ones (4: one
// dword load per tap and one 16-byte store; 1: rows or a source pointer that are not dword-aligned).  left / count / the
// weights are uniform over the workgroup (scalar loads).  A workgroup walks kVerticalRows neighbouring output rows of its
// column strip, so the source rows they share are re-read from L1 / L2.
template <int VEC>
__global__ __launch_bounds__(256) void lanczos3_vertical_kernel(const uint8_t* __restrict__ src, int64_t row_bytes,
                                                                float* __restrict__ mid, const int2* __restrict__ span,
                                                                const float* __restrict__ wt, int len_out) {
    const int64_t col = ((int64_t)blockIdx.y * 256 + threadIdx.x) * VEC;
    if (col >= row_bytes) return;
    const int o0 = blockIdx.x * kVerticalRows;
    const int o1 = min(o0 + kVerticalRows, len_out);
    for (int o = o0; o < o1; ++o) {
        const int2 sp = span[o];
        const uint8_t* p = src + (int64_t)sp.x * row_bytes + col;
        const float* w = wt + o;
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.0f;
#pragma unroll 4
        for (int i = 0; i < sp.y; ++i) {
            const float wi = w[(int64_t)i * len_out];
            if constexpr (VEC == 4) {
                const uint32_t px = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn((float)((px >> (8 * j)) & 255u), wi));
            } else {
                acc[0] = __fadd_rn(acc[0], __fmul_rn((float)p[0], wi));
            }
            p += row_bytes;
        }
        float* out = mid + (int64_t)o * row_bytes + col;
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else
            out[0] = acc[0];
    }
}

// FloatNearest of the crate: clamp to the sample range, then f32::round (half away from zero)
__device__ __forceinline__ uint8_t to_u8(float t) {
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (uint8_t)roundf(t);
}

// Horizontal pass.  A workgroup owns `run` neighbouring output pixels of one row, one per lane.  STAGED: the floats of
// the intermediate row those pixels read, [3 * left(first), 3 * right(last)), are staged into LDS first (left and right
// never decrease with the output index), with 16-byte loads where the row length allows.  Not STAGED: downscales whose
// span does not fit read the intermediate from global memory.  The run's bytes are collected in LDS and stored as whole
// dwords between an unaligned head and tail.
template <bool STAGED>
__global__ __launch_bounds__(256) void lanczos3_horizontal_kernel(const float* __restrict__ mid, int w_in,
                                                                  uint8_t* __restrict__ dst, int nw,
                                                                  const int2* __restrict__ span,
                                                                  const float* __restrict__ wt, int run) {
    extern __shared__ __attribute__((aligned(16))) float staged[];
    __shared__ uint8_t obytes[256 * 3];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y;
    const int o0 = blockIdx.x * run;
    const int n = min(run, nw - o0);
    const float* line = mid + row * w_in * 3;
    int base = 0;
    if constexpr (STAGED) {
        const int2 s0 = span[o0], s1 = span[o0 + n - 1];
        int f0 = s0.x * 3, f1 = (s1.x + s1.y) * 3;
        if ((w_in & 3) == 0) {
            // rows of 3 * w_in floats start 16-byte aligned and hold a whole number of float4
            f0 &= ~3, f1 = (f1 + 3) & ~3;
            const float4* line4 = reinterpret_cast<const float4*>(line);
            float4* staged4 = reinterpret_cast<float4*>(staged);
            for (int k = f0 / 4 + tid; k < f1 / 4; k += blockDim.x) staged4[k - f0 / 4] = line4[k];
        } else {
            for (int k = f0 + tid; k < f1; k += blockDim.x) staged[k - f0] = line[k];
        }
        base = f0;
        __syncthreads();
    }
    if (tid < n) {
        const int o = o0 + tid;
        const int2 sp = span[o];
        const float* p = STAGED ? staged + (sp.x * 3 - base) : line + sp.x * 3;
        const float* w = wt + o;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        for (int i = 0; i < sp.y; ++i) {
            const float wi = w[(int64_t)i * nw];
            r = __fadd_rn(r, __fmul_rn(p[0], wi));
            g = __fadd_rn(g, __fmul_rn(p[1], wi));
            b = __fadd_rn(b, __fmul_rn(p[2], wi));
            p += 3;
        }
        obytes[3 * tid + 0] = to_u8(r);
        obytes[3 * tid + 1] = to_u8(g);
        obytes[3 * tid + 2] = to_u8(b);
    }
    __syncthreads();
    uint8_t* out = dst + (row * nw + o0) * 3;
    const int nbytes = n * 3;
    const int lead = min((int)((4 - (reinterpret_cast<uintptr_t>(out) & 3)) & 3), nbytes);
    const int ndw = (nbytes - lead) / 4;
    const int tail = lead + 4 * ndw;
    if (tid < lead) out[tid] = obytes[tid];
    for (int k = tid; k < ndw; k += blockDim.x) {
        const int at = lead + 4 * k;
        const uint32_t v = (uint32_t)obytes[at] | ((uint32_t)obytes[at + 1] << 8) | ((uint32_t)obytes[at + 2] << 16) |
                           ((uint32_t)obytes[at + 3] << 24);
        *reinterpret_cast<uint32_t*>(out + at) = v;
    }
    if (tid < nbytes - tail) out[tail + tid] = obytes[tail + tid];
}

// The (len_in, len_out) table on the device: built once, kept in the context.  A full cache loses its least recently
// used entry, behind a synchronise of both streams of the context: a queued kernel may still read it.
ResampleTable resample_table(me_ctx* ctx, int32_t len_in, int32_t len_out) {
    for (ResampleTable& t : ctx->rs_tables)
        if (t.len_in == len_in && t.len_out == len_out) {
            t.stamp = ++ctx->rs_stamp;
            return t;
        }
    const int64_t nweights = lanczos3_table_weights(len_in, len_out);
    ME_CHECK(nweights > 0, ME_ERR_BAD_SHAPE, "Lanczos3 table %d -> %d", len_in, len_out);
    std::vector<int32_t> left(len_out), count(len_out);
    std::vector<float> packed((size_t)nweights);
    lanczos3_table_fill(len_in, len_out, left.data(), count.data(), packed.data());
    int32_t taps = 0;
    for (int32_t c : count) taps = std::max(taps, c);
    std::vector<int2> span(len_out);
    std::vector<float> wt((size_t)taps * len_out, 0.0f);
    const float* ws = packed.data();
    for (int32_t o = 0; o < len_out; ++o) {
        span[o] = make_int2(left[o], count[o]);
        for (int32_t i = 0; i < count[o]; ++i) wt[(size_t)i * len_out + o] = ws[i];
        ws += count[o];
    }
    ResampleTable t;
    t.len_in = len_in, t.len_out = len_out;
    // the longest run of output pixels whose staged span (with the float4 rounding at both ends) fits the LDS
    for (int run = 256; run >= 32 && !t.run; run /= 2) {
        int need = 0;
        for (int32_t o0 = 0; o0 < len_out; o0 += run) {
            const int32_t o1 = std::min(o0 + run, len_out) - 1;
            const int f0 = (left[o0] * 3) & ~3, f1 = ((left[o1] + count[o1]) * 3 + 3) & ~3;
            need = std::max(need, f1 - f0);
        }
        if (need <= kLdsFloats) t.run = run, t.lds_floats = need;
    }
    if (ctx->rs_tables.size() >= me_ctx::kMaxResampleTables) {
        ME_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->own_stream) ME_HIP(hipStreamSynchronize(ctx->own_stream));
        if (ctx->out_stream) ME_HIP(hipStreamSynchronize(ctx->out_stream));
        auto victim = std::min_element(ctx->rs_tables.begin(), ctx->rs_tables.end(),
                                       [](const ResampleTable& a, const ResampleTable& b) { return a.stamp < b.stamp; });
        (void)hipFree(victim->span);
        (void)hipFree(victim->w);
        ctx->rs_tables.erase(victim);
    }
    // fresh allocations that nothing queued reads, filled by blocking copies: valid for every later launch
    ME_HIP(hipMalloc((void**)&t.span, span.size() * sizeof(int2)));
    if (hipMalloc((void**)&t.w, wt.size() * sizeof(float)) != hipSuccess) {
        (void)hipFree(t.span);
        fail(ME_ERR_OOM, "Lanczos3 table %d -> %d: %zu bytes", len_in, len_out, wt.size() * sizeof(float));
    }
    const hipError_t e1 = hipMemcpy(t.span, span.data(), span.size() * sizeof(int2), hipMemcpyHostToDevice);
    const hipError_t e2 = hipMemcpy(t.w, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e1 != hipSuccess || e2 != hipSuccess) {
        (void)hipFree(t.span);
        (void)hipFree(t.w);
        ME_HIP(e1);
        ME_HIP(e2);
    }
    t.stamp = ++ctx->rs_stamp;
    ctx->rs_tables.push_back(t);
    return t;
}

}  // namespace

void free_resample_tables(me_ctx* ctx) {
    for (ResampleTable& t : ctx->rs_tables) {
        (void)hipFree(t.span);
        (void)hipFree(t.w);
    }
    ctx->rs_tables.clear();
}

void resize_lanczos3_rgb8(me_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst, int32_t nw, int32_t nh) {
    hipStream_t s = ctx->stream;
    if (w == nw && h == nh) {  // imageops::resize: the same size is a copy
        ME_HIP(hipMemcpyAsync(dst, src, (size_t)w * h * 3, hipMemcpyDeviceToDevice, s));
        return;
    }
    // the output back end may run on its own stream (me_ctx_set_output_overlap): its intermediate is its own
    const bool on_out = ctx->out_stream && s == ctx->out_stream;
    float* mid = (float*)site_buf(ctx, on_out ? "out.resample.mid" : "resample.mid", (size_t)w * nh * 3 * sizeof(float));
    const ResampleTable tv = resample_table(ctx, h, nh);
    const ResampleTable th = resample_table(ctx, w, nw);

    const int64_t row_bytes = (int64_t)w * 3;
    const bool vec = (row_bytes & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    const dim3 vgrid((unsigned)cdiv(nh, kVerticalRows), (unsigned)cdiv(row_bytes, vec ? 1024 : 256));
    if (vec)
        hipLaunchKernelGGL(lanczos3_vertical_kernel<4>, vgrid, dim3(256), 0, s, src, row_bytes, mid, tv.span, tv.w, nh);
    else
        hipLaunchKernelGGL(lanczos3_vertical_kernel<1>, vgrid, dim3(256), 0, s, src, row_bytes, mid, tv.span, tv.w, nh);
    ME_HIP(hipGetLastError());

    if (th.run) {
        const dim3 hgrid((unsigned)cdiv(nw, th.run), (unsigned)nh);
        hipLaunchKernelGGL(lanczos3_horizontal_kernel<true>, hgrid, dim3(std::max(th.run, 64)),
                           (size_t)th.lds_floats * sizeof(float), s, mid, w, dst, nw, th.span, th.w, th.run);
    } else {
        const int run = 64;
        const dim3 hgrid((unsigned)cdiv(nw, run), (unsigned)nh);
        hipLaunchKernelGGL(lanczos3_horizontal_kernel<false>, hgrid, dim3(run), 0, s, mid, w, dst, nw, th.span, th.w, run);
    }
    ME_HIP(hipGetLastError());
}

}  // namespace me
