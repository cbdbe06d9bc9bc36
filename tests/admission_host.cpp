// Host driver of csrc/admission.h for tests/test_admission_cpu.py: the header (and through it gemm_params.h) and nothing else of the
// library.  Reads one case per line from stdin (tests/admission_cases.py writes the lines) and prints "0" where the call is admitted,
// "<code>\t<message>" where it is refused.  A descriptor is built through the gemm_params.h builders, as pipeline.hip and api.hip
// build theirs; pointers are small fake non-null integers and are never dereferenced.
//   g <form> key=value ...   admit_gemm (form hc: admit_head_composed) of the descriptor `form` builds from the keys (defaults below),
//                            then `p.<member>=<value>` sets a member directly, in the order given; amode= / epi= override the form's
//      lin   linear_params            M N K A W bias out16 out32 act | parts16 (set_out16_parts) qcols (set_scaled_cols) seg1 seg2 ln ln8
//      res   resid_params             M N K A W bias gamma x32       | seg1 seg2 ln (set_fused_layernorm) ln8 (its fp8 output)
//      pe    patch_embed_params       windows P C
//      conv  conv_params              B H W Cin Cout k stride bias out32 out16 border16 parts16 act act16_only res32 res32b tap_bias a_split
//      convt convt_params             B H W Cin Cout bias out32 out16 border16 pixel_stride act16 out_split lo_off a_wrap (set_a_wrap)
//      pair  chain_convt              B H W Cout Cin_a Cin_b a_wrap_b bias_b border16 act16
//      hf    head_final_params        B H W Cin Cmid
//      hc    head_composed_params     B H W Cin tap_bias
//   f <form> key=value ...   admit_gemm_fp8: lin / res as above with set_fp8_operands; out8 (set_out8), seg1 seg2, ln
//   a windows tokens heads out8 out8_scale out8_mt                         admit_attention
//   q rows K weight_layout                                                 admit_quantize_fp8
//   o <entry> <ints ...>     the rule of a me_op_* entry, the arguments in the order of its admit_op_* function; an array of three
//                            pointers is given as the bit mask of its NULL members, a single pointer as 0 / 1
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "../matrix-eyes_amd/csrc/admission.h"

namespace me {
void fail(int32_t code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error{code, buf};
}
}  // namespace me

using namespace me;

namespace {

// fake operands: distinct, non-null, never dereferenced
template <class T>
T* fake(int n) { return (T*)(uintptr_t)(0x1000 + 0x100 * n); }
template <class T>
T* fake_if(long long on, int n) { return on ? fake<T>(n) : nullptr; }

struct Args {
    std::map<std::string, long long> kv;
    std::vector<std::pair<std::string, long long>> members;  // p.<member>=<value>, in order
    long long get(const char* k, long long dflt) const {
        auto it = kv.find(k);
        return it == kv.end() ? dflt : it->second;
    }
};

bool set_member(GemmParams& p, const std::string& name, long long v) {
#define ME_INT(m) if (name == #m) { p.m = (decltype(p.m))v; return true; }
#define ME_PTR(m) if (name == #m) { p.m = v ? fake<std::remove_pointer<decltype(p.m)>::type>(64 + (int)v) : nullptr; return true; }
    ME_INT(M) ME_INT(N) ME_INT(K) ME_INT(lda) ME_INT(in_Hp) ME_INT(in_Wp) ME_INT(Cin) ME_INT(out_H) ME_INT(out_W) ME_INT(KH) ME_INT(KW)
    ME_INT(stride) ME_INT(ldc) ME_INT(ldc16) ME_INT(lo_off16) ME_INT(hi2_off16) ME_INT(act) ME_INT(act16_only) ME_INT(out16_border)
    ME_INT(tokens_per_window) ME_INT(Cout) ME_INT(pixels_per_image) ME_INT(seg1) ME_INT(seg2) ME_INT(a_mt) ME_INT(out8_mt) ME_INT(qcols)
    ME_INT(a_wrap) ME_INT(lda2) ME_INT(K2) ME_INT(a_wrap2)
    ME_PTR(A) ME_PTR(W) ME_PTR(bias) ME_PTR(gamma) ME_PTR(res32) ME_PTR(res32b) ME_PTR(pos) ME_PTR(out32) ME_PTR(out16) ME_PTR(tap_bias)
    ME_PTR(w2) ME_PTR(b2) ME_PTR(W_s1) ME_PTR(W_s2) ME_PTR(bias_s1) ME_PTR(bias_s2) ME_PTR(gamma_s1) ME_PTR(gamma_s2) ME_PTR(a_scale)
    ME_PTR(w_scale) ME_PTR(w_scale_s1) ME_PTR(w_scale_s2) ME_PTR(out8) ME_PTR(out8_scale) ME_PTR(ln_out16) ME_PTR(ln_w) ME_PTR(ln_b)
    ME_PTR(ln_w_s1) ME_PTR(ln_b_s1) ME_PTR(ln_w_s2) ME_PTR(ln_b_s2) ME_PTR(ln_stats) ME_PTR(ln_count) ME_PTR(A2) ME_PTR(W2) ME_PTR(bias2)
#undef ME_INT
#undef ME_PTR
    return false;
}

// what the row-segmented launches add to a linear / residual descriptor: every set of the three segments present
void add_segments_and_ln(GemmParams& p, const Args& a, bool fp8) {
    if (a.kv.count("seg1") || a.kv.count("seg2")) {
        SegWeights w;
        for (int i = 0; i < 3; ++i) {
            w.W[i] = fake<void>(10 + i), w.bias[i] = fake<float>(13 + i), w.gamma[i] = fake<float>(16 + i);
            w.w_scale[i] = fp8 ? fake<uint8_t>(19 + i) : nullptr;
        }
        set_segments(p, a.get("seg1", 0), a.get("seg2", 0), w);
    }
    if (a.get("ln", 0)) {
        const LnSet ln{fake<float>(22), fake<float>(23), fake<float>(24), fake<float>(25), fake<float>(26), fake<float>(27)};
        const bool ln8 = a.get("ln8", 0) != 0;
        set_fused_layernorm(p, ln, 1e-6f, ln8 ? nullptr : fake<void>(28), ln8 ? fake<uint8_t>(29) : nullptr,
                            ln8 ? fake<uint8_t>(30) : nullptr, fake<unsigned long long>(31), fake<unsigned>(32));
    }
}

GemmParams build(const std::string& form, const Args& a, bool fp8, AMode& amode, EpiKind& epi) {
    amode = A_PLAIN, epi = EPI_STORE;
    GemmParams p = base_params();
    const int M = (int)a.get("M", 64), N = (int)a.get("N", 64), K = (int)a.get("K", fp8 ? 256 : 64);
    const int B = (int)a.get("B", 1), H = (int)a.get("H", 8), W = (int)a.get("W", 8), Cin = (int)a.get("Cin", 64);
    if (form == "lin") {
        p = linear_params(M, N, K, fake_if<void>(a.get("A", 1), 1), fake_if<void>(a.get("W", 1), 2), fake_if<float>(a.get("bias", 1), 3),
                          fake_if<void>(a.get("out16", 1), 4), fake_if<float>(a.get("out32", 0), 5), (int)a.get("act", ACT_NONE));
        if (a.kv.count("parts16")) set_out16_parts(p, N, (int)a.get("parts16", 1));
        if (a.kv.count("qcols")) set_scaled_cols(p, (int)a.get("qcols", 0), kAttnQScale);
    } else if (form == "res") {
        epi = EPI_RESID_SCALE;
        p = resid_params(M, N, K, fake_if<void>(a.get("A", 1), 1), fake_if<void>(a.get("W", 1), 2), fake_if<float>(a.get("bias", 1), 3),
                         fake_if<float>(a.get("gamma", 1), 6), fake_if<float>(a.get("x32", 1), 5));
    } else if (form == "pe") {
        epi = EPI_PATCH_EMBED;
        p = patch_embed_params((int)a.get("windows", 2), (int)a.get("P", 64), (int)a.get("C", 64), fake<void>(1), fake<void>(2), fake<float>(3),
                               fake<float>(7), fake<float>(5));
    } else if (form == "conv") {
        amode = A_CONV;
        ConvOut o;
        o.out32 = fake_if<float>(a.get("out32", 1), 5), o.out16 = fake_if<void>(a.get("out16", 0), 4), o.border16 = a.get("border16", 0) != 0;
        o.parts16 = (int)a.get("parts16", 1), o.act = (int)a.get("act", ACT_NONE), o.act16_only = a.get("act16_only", 1) != 0;
        o.res32 = fake_if<float>(a.get("res32", 0), 8), o.res32b = fake_if<float>(a.get("res32b", 0), 9);
        o.tap_bias = fake_if<float>(a.get("tap_bias", 0), 33);
        p = conv_params(fake<void>(1), B, H, W, Cin, fake<void>(2), (int)a.get("Cout", 64), (int)a.get("k", 3), (int)a.get("stride", 1),
                        fake_if<float>(a.get("bias", 1), 3), o, a.get("a_split", 0) != 0);
    } else if (form == "convt") {
        epi = EPI_CONVT;
        p = convt_params(fake<void>(1), B, H, W, Cin, fake<void>(2), (int)a.get("Cout", 8), fake_if<float>(a.get("bias", 1), 3),
                         fake_if<float>(a.get("out32", 1), 5), fake_if<void>(a.get("out16", 0), 4), a.get("border16", 0) != 0,
                         a.get("pixel_stride", 0), (int)a.get("act16", ACT_NONE), false, a.get("out_split", 0) != 0, a.get("lo_off", 0));
        if (a.get("a_wrap", 0)) set_a_wrap(p, (int)a.get("a_wrap", 0));
    } else if (form == "pair") {
        epi = EPI_CONVT;
        const int Cout = (int)a.get("Cout", 8);
        const GemmParams first = convt_params(fake<void>(1), B, H, W, (int)a.get("Cin_a", 64), fake<void>(2), Cout, nullptr, nullptr, fake<void>(4),
                                              a.get("border16", 0) != 0, 0, (int)a.get("act16", ACT_NONE));
        GemmParams second = convt_params(fake<void>(34), B, H, W, (int)a.get("Cin_b", 128), fake<void>(35), Cout,
                                         fake_if<float>(a.get("bias_b", 1), 36), nullptr, nullptr, false, 0, ACT_NONE);
        if (a.get("a_wrap_b", 0)) set_a_wrap(second, (int)a.get("a_wrap_b", 0));
        p = chain_convt(first, second, fake<float>(5));
    } else if (form == "hf") {
        amode = A_CONV, epi = EPI_HEAD_FINAL;
        p = head_final_params(fake<void>(1), B, H, W, Cin, fake<void>(2), (int)a.get("Cmid", 32), fake<float>(3), fake<float>(37), fake<float>(38),
                              nullptr, 1e-4f, 1e4f, fake<float>(5));
    } else if (form == "hc") {
        amode = A_CONV, epi = EPI_HEAD_COMPOSED;
        p = head_composed_params(fake<void>(1), B, H, W, Cin, fake<void>(2), fake<float>(3), fake_if<float>(a.get("tap_bias", 1), 33),
                                 fake<float>(37), fake<float>(38), nullptr, 1e-4f, 1e4f, fake<float>(5));
    } else {
        exit(2);
    }
    if (fp8) {
        set_fp8_operands(p, fake<uint8_t>(39), fake<uint8_t>(40));
        if (a.get("out8", 0)) p.out16 = nullptr, p.act = ACT_GELU, set_out8(p, fake<uint8_t>(41), fake<uint8_t>(42));
    }
    add_segments_and_ln(p, a, fp8);
    for (const auto& m : a.members)
        if (!set_member(p, m.first, m.second)) exit(2);
    if (a.kv.count("amode")) amode = (AMode)a.get("amode", 0);
    if (a.kv.count("epi")) epi = (EpiKind)a.get("epi", 0);
    return p;
}

// an array of three pointers whose members named in null_mask are null
template <class T>
struct Three {
    const T* v[3];
    Three(long long null_mask, int n) {
        for (int i = 0; i < 3; ++i) v[i] = (null_mask >> i) & 1 ? nullptr : fake<T>(n + i);
    }
};

void op(const std::string& e, const std::vector<long long>& v) {
    auto I = [&](size_t i) { if (i >= v.size()) exit(2); return (int32_t)v[i]; };
    auto L = [&](size_t i) { if (i >= v.size()) exit(2); return (int64_t)v[i]; };
    if (e == "conv2d") admit_op_conv2d(I(0), I(1));
    else if (e == "head_final") admit_op_head_final(I(0), I(1), I(2), I(3), I(4));
    else if (e == "conv2d_forms") admit_op_conv2d_forms(I(0), I(1), I(2), I(3), I(4), I(5), I(6), fake_if<void>(L(7), 4), I(8), I(9));
    else if (e == "convt_forms") admit_op_conv_transpose2x2_forms(I(0), I(1), I(2), I(3), I(4), I(5), fake_if<void>(L(6), 4), I(7), I(8), I(9), I(10));
    else if (e == "convt_pair") admit_op_conv_transpose2x2_pair(I(0), I(1), I(2), I(3), I(4), I(5), I(6), I(7), I(8));
    else if (e == "patch_embed") admit_op_patch_embed(I(0), I(1), I(2));
    else if (e == "linear_segments") {
        const Three<void> W(L(3), 10);
        const Three<float> g(L(4), 16);
        admit_op_linear_segments(I(0), I(1), I(2), W.v, L(4) == 8 ? nullptr : g.v, L(5) != 0);  // (mask 8: no gamma array at all)
    } else if (e == "lrl" || e == "lrl_fp8") {
        const Three<void> W(L(4), 10);
        const Three<float> b(L(5), 13), g(L(6), 16), lw(L(7), 22), lb(L(8), 25);
        admit_op_linear_residual_layernorm(e == "lrl" ? "me_op_linear_residual_layernorm" : "me_op_linear_residual_layernorm_fp8", I(0), I(1), I(2),
                                           I(3), W.v, b.v, g.v, lw.v, lb.v);
    } else if (e == "fp8_rl_weights") {
        const Three<uint8_t> W(L(2), 10), ws(L(3), 19);
        const Three<float> b(L(4), 13), g(L(5), 16), lw(L(6), 22), lb(L(7), 25);
        admit_segment_weights("me_op_linear_fp8_residual_layernorm", L(0), L(1), W.v, ws.v, b.v, g.v, lw.v, lb.v);
    } else if (e == "attention_segments") {
        admit_op_attention_segments(fake_if<uint8_t>(L(0), 41), I(1), I(2), I(3), L(4), L(5), L(6), I(7), I(8));
    } else if (e == "layernorm_segments") {
        const Three<float> w(L(0), 22), b(L(1), 25);
        admit_op_layernorm_segments(w.v, b.v, L(2), L(3), fake_if<uint8_t>(L(4), 41), L(5), I(6));
    } else if (e == "map") admit_map("me_op_nchw32_to_nhwc", I(0), I(1), I(2), I(3));
    else if (e == "bilinear") admit_op_bilinear(I(0), I(1), I(2));
    else if (e == "patchify") admit_op_patchify(I(0), I(1));
    else if (e == "patchify_windows") admit_op_patchify_windows(I(0), I(1));
    else if (e == "cls_rows") admit_op_cls_rows(I(0), I(1), I(2));
    else if (e == "merge") admit_op_merge(I(0), I(1), I(2), I(3), I(4), I(5), I(6));
    else if (e == "concat_channels") admit_op_concat_channels(L(0), I(1), I(2));
    else if (e == "fov_add") admit_op_fov_add(I(0), I(1), I(2), I(3));
    else if (e == "fov_final") admit_op_fov_final(I(0), I(1), I(2));
    else exit(2);
}

void run(const std::string& line) {
    std::istringstream in(line);
    std::string kind, form, tok;
    in >> kind;
    if (kind == "g" || kind == "f") {
        in >> form;
        Args a;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) exit(2);
            const long long v = atoll(tok.c_str() + eq + 1);
            if (tok.compare(0, 2, "p.") == 0) a.members.emplace_back(tok.substr(2, eq - 2), v);
            else a.kv[tok.substr(0, eq)] = v;
        }
        AMode amode;
        EpiKind epi;
        const GemmParams p = build(form, a, kind == "f", amode, epi);
        if (kind == "f") admit_gemm_fp8(p, epi);
        else if (form == "hc") admit_head_composed(p);
        else admit_gemm(p, amode, epi);
        return;
    }
    std::vector<long long> v;
    if (kind == "o") in >> form;
    while (in >> tok) v.push_back(atoll(tok.c_str()));
    if (kind == "a" && v.size() == 6) admit_attention((int32_t)v[0], (int32_t)v[1], (int32_t)v[2], fake_if<uint8_t>(v[3], 41), fake_if<uint8_t>(v[4], 42), v[5]);
    else if (kind == "q" && v.size() == 3) admit_quantize_fp8(v[0], (int32_t)v[1], (int32_t)v[2]);
    else if (kind == "o") op(form, v);
    else exit(2);
}

}  // namespace

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '\n') continue;
        try {
            run(line);
            printf("0\n");
        } catch (const Error& e) {
            printf("%d\t%s\n", e.code, e.msg.c_str());
        }
    }
    return 0;
}
