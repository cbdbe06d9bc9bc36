// Per-axis Lanczos3 weight table of `image` 0.25.10 imageops/sample.rs (vertical_sample / horizontal_sample), built on
// the host for the kernels of resample.hip.
//
// Plain C++, compiled by g++ with -ffp-contract=off and neither fast-math nor a vector math library (Makefile): the
// table has to come out bit for bit as safe Rust computes it.  `((float)o + 0.5f) * ratio - 0.5f` or
// `center - 3.0f * sratio` contracted into an FMA moves `left` and the weights, and the sine is libm's scalar sinf
// (Rust's f32::sin on this platform) -- the device's sine is another function and would cost the last bit.
#include <cmath>
#include <cstdint>

#include "lanczos_table.h"

namespace {

float sinc(float t) {
    if (t == 0.0f) return 1.0f;
    const float a = t * 3.14159265358979323846f;
    return sinf(a) / a;
}
float lanczos3_kernel(float x) { return fabsf(x) < 3.0f ? sinc(x) * sinc(x / 3.0f) : 0.0f; }

struct Span {
    int64_t left, right;
    float center;  // already moved by -0.5
};

Span span_of(int64_t o, int64_t len_in, float ratio, float src_support) {
    float center = ((float)o + 0.5f) * ratio;
    int64_t left = (int64_t)floorf(center - src_support);
    if (left < 0) left = 0;
    if (left > len_in - 1) left = len_in - 1;
    int64_t right = (int64_t)ceilf(center + src_support);
    if (right < left + 1) right = left + 1;
    if (right > len_in) right = len_in;
    return {left, right, center - 0.5f};
}

}  // namespace

namespace me {

int64_t lanczos3_table_weights(int32_t len_in, int32_t len_out) {
    if (len_in < 1 || len_out < 1 || len_in > ME_RESIZE_MAX_DIM || len_out > ME_RESIZE_MAX_DIM) return -1;
    const float ratio = (float)len_in / (float)len_out;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = 3.0f * sratio;
    int64_t n = 0;
    for (int64_t o = 0; o < len_out; ++o) {
        const Span s = span_of(o, len_in, ratio, src_support);
        n += s.right - s.left;
    }
    return n;
}

void lanczos3_table_fill(int32_t len_in, int32_t len_out, int32_t* left, int32_t* count, float* weights) {
    const float ratio = (float)len_in / (float)len_out;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = 3.0f * sratio;
    float* ws = weights;
    for (int64_t o = 0; o < len_out; ++o) {
        const Span s = span_of(o, len_in, ratio, src_support);
        const int64_t n = s.right - s.left;
        float sum = 0.0f;
        for (int64_t i = 0; i < n; ++i) {
            const float w = lanczos3_kernel(((float)(s.left + i) - s.center) / sratio);
            ws[i] = w;
            sum += w;
        }
        for (int64_t i = 0; i < n; ++i) ws[i] /= sum;
        left[o] = (int32_t)s.left, count[o] = (int32_t)n;
        ws += n;
    }
}

}  // namespace me

extern "C" int64_t me_op_lanczos3_table(int32_t len_in, int32_t len_out, int32_t* left, int32_t* count, float* weights,
                                        int64_t weights_cap) {
    const int64_t need = me::lanczos3_table_weights(len_in, len_out);
    if (need < 0) return -1;
    if (weights_cap < need) return need;
    if (!left || !count || !weights) return -1;
    me::lanczos3_table_fill(len_in, len_out, left, count, weights);
    return need;
}
