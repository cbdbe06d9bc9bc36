"""The cases of tests/test_admission_cpu.py: one line each for tests/admission_host.cpp, which builds the descriptor the line names
through the csrc/gemm_params.h builders and asks csrc/admission.h whether the launcher or the entry takes it.

For every ME_CHECK clause of admission.h, for each disjunct of its condition, one case that passes every earlier clause and fails on
that disjunct, and the admitted neighbour one step away -- at the smallest shapes at which the rule can bite (M = N = K = 64, an 8 x 8
map with Cin = 64; the fp8 GEMM from N = K = 256), never the model's own.  Where the 16-bit launcher admits what the fp8 launcher
refuses (a row segment without weights, segment starts beyond M) both answers are in the table: the difference is kept.

The answers are tests/golden/admission_table.txt: the output of the checks as they stood in gemm.hip, gemm_fp8.hip, attention.hip and
api.hip before csrc/admission.h existed, cut verbatim into a host program and run over this list, stored one to a line beside the
digest of the list.  The header is held to that table, not the other way round.  A new rule gets its cases HERE first, and its
answers from the code the rule is cut out of."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = []


def g(form, *kv):
    CASES.append(" ".join(("g", form) + kv))


def f(form, *kv):
    CASES.append(" ".join(("f", form) + kv))


def o(entry, *ints):
    CASES.append(" ".join(["o", entry] + [str(int(i)) for i in ints]))


M = 64
BOUNDS = [0, 16, 24, 256, M, M + 16]                  # row-segment starts, asked in both orders
PAIRS = [(a, b) for a in BOUNDS for b in BOUNDS]

# ---- admit_gemm -------------------------------------------------------------------------------------------
g("lin")
for m, n, k in [(0, 64, 64), (64, 0, 64), (64, 64, 0), (1, 64, 64), (64, 64, 32), (64, 64, 96), (64, 64, 128)]:
    g("lin", "M=%d" % m, "N=%d" % n, "K=%d" % k)
for n in (4, 6, 256, 768, 1024, (1 << 30) - 4, 1 << 30):
    g("lin", "N=%d" % n)
for m in ((1 << 30) - 1, 1 << 30):
    g("lin", "M=%d" % m)
g("lin", "A=0")
g("lin", "W=0")
g("lin", "bias=0")                                    # (no rule asks for a bias)
# the convolution operand
g("conv")
g("conv", "k=1")
g("conv", "a_split=1", "Cin=32")
g("conv", "k=1", "p.Cin=32", "p.KH=2")                # Cin % 64 alone (K = KH * KW * Cin holds)
g("conv", "k=1", "p.K=128")                           # K alone
g("conv", "p.out_H=0")
g("conv", "p.out_W=0")
g("conv", "p.out_H=5")                                # M = 64 is no multiple of 5 x 8
g("conv", "stride=2")
# a_wrap and lda of a plain operand
for k in (64, 128):
    for lda in (k - 8, k, k + 4, k + 8):
        g("lin", "K=%d" % k, "p.lda=%d" % lda)
g("lin", "p.a_wrap=-1")
g("lin", "K=128", "p.a_wrap=2")
g("lin", "K=128", "p.a_wrap=1", "p.lda=64")           # a wrapped operand is the ConvTranspose's only
g("convt", "Cin=128")
g("convt", "Cin=128", "a_wrap=64")                    # at the limit: the second half wraps onto the first
g("convt", "Cin=192", "a_wrap=64")                    # past it
g("convt", "Cin=192", "a_wrap=128")
g("convt", "Cin=128", "a_wrap=64", "p.lda=56")
g("convt", "Cin=128", "a_wrap=64", "p.lda=68")
g("convt", "Cin=128", "a_wrap=64", "p.lda=72")
# the ConvTranspose's Cout
for cout in (4, 6, 8, 12):
    g("convt", "Cout=%d" % cout)
g("convt", "p.Cout=0")
g("convt", "p.Cout=-4")
# a chained operand set: each forbidden member in turn
g("pair")
for m in ("p.W2=0", "p.out16=0", "p.out32=0", "p.bias=1", "p.lo_off16=8", "p.seg1=64", "p.act=1", "p.act=2", "p.hi2_off16=8"):
    g("pair", m)
for m in (("p.K2=0",), ("p.K2=32",), ("p.a_wrap2=-1",), ("p.a_wrap2=2",), ("p.a_wrap2=1",), ("p.lda2=124",), ("p.lda2=120",), ("p.lda2=136",),
          ("a_wrap_b=64",), ("Cin_b=192", "a_wrap_b=64"), ("Cin_b=192", "a_wrap_b=128"), ("a_wrap_b=64", "p.lda2=56"), ("a_wrap_b=64", "p.lda2=68")):
    g("pair", *m)
for cout in (4, 8, 12, 16):
    g("pair", "Cout=%d" % cout)
# the head's final layers
for cmid in (4, 32, 36):
    g("hf", "Cmid=%d" % cmid)
g("hc", "H=16", "W=16")
for m in ("p.N=64", "p.KH=1", "p.KW=1", "p.stride=2", "p.Cin=32", "p.K=640", "p.out_H=8", "p.out_W=8", "p.M=128", "p.M=320", "tap_bias=0",
          "p.A=0", "p.W=0", "p.bias=0", "p.w2=0", "p.b2=0", "p.out32=0", "p.pixels_per_image=256"):
    g("hc", "H=16", "W=16", m)
# per-tap bias shares: each excluded option in turn
TAP = ("tap_bias=1", "out16=1", "border16=1", "out32=0")
g("conv", *TAP)
g("conv", *TAP, "act=2")
for m in (("amode=0", "p.lda=576"), ("epi=1",), ("k=1",), ("p.KW=1", "p.K=192"), ("stride=2",), ("p.out16=0",), ("border16=0",), ("bias=0",),
          ("Cout=4",), ("Cout=8",), ("out32=1",), ("res32=1",), ("res32b=1",), ("parts16=2",), ("p.hi2_off16=128",), ("act=1",)):
    g("conv", *TAP, *m)
# the fused LayerNorm
LN = ("N=256", "K=128", "ln=1")
g("res", *LN)
for n in (128, 512, 768, 1024):
    g("res", "N=%d" % n, "K=128", "ln=1")
for m in ("p.ldc=512", "p.ln_w=0", "p.ln_b=0", "p.ln_stats=0", "p.ln_count=0", "p.bias=0", "p.gamma=0", "p.res32=0", "p.out32=0"):
    g("res", *LN, m)
for m in ("p.ln_w_s1=0", "p.ln_b_s1=0", "p.ln_w_s2=0", "p.ln_b_s2=0", "p.W_s1=0", "p.bias_s1=0", "p.gamma_s1=0"):
    g("res", *LN, "seg1=16", m)
    g("res", *LN, "seg1=16", "seg2=24", m.replace("s1", "s2") if "ln_" not in m else m)
g("res", *LN, "ln8=1")
g("res", *LN, "ln8=1", "p.out8_scale=0")
g("res", *LN, "ln8=1", "p.out8_mt=0")
g("res", *LN, "ln8=1", "M=129")
g("res", *LN, "ln8=1", "M=129", "p.out8_mt=1")
for a, b in PAIRS:                                    # (the starts themselves are the tile's business: tile_choice.h config_refusal)
    g("res", "seg1=%d" % a, "seg2=%d" % b)
# scaled leading columns
for q in (0, 32, 64, 128, 128 + 64):
    g("lin", "N=128", "qcols=%d" % q)
for m in (("out16=0", "out32=1"), ("out32=1",), ("act=2",), ("act=1",), ("parts16=2",), ("p.hi2_off16=128",), ("epi=4", "p.Cout=32")):
    g("lin", "N=128", "qcols=64", *m)
g("res", "N=128", "p.qcols=64")

# ---- admit_gemm_fp8 ---------------------------------------------------------------------------------------
F = ("N=256",)
f("lin", *F)
for m, n, k in [(0, 256, 256), (64, 0, 256), (64, 128, 256), (64, 768, 256), (64, 256, 128), (64, 256, 320), (64, 256, 384), (1, 256, 256)]:
    f("lin", "M=%d" % m, "N=%d" % n, "K=%d" % k)
for m in ("A=0", "W=0", "p.a_scale=0", "p.w_scale=0"):
    f("lin", *F, m)
f("lin", *F, "M=129")
f("lin", *F, "M=129", "p.a_mt=1")                     # one tile of A scales short
for lda in (240, 256, 264, 272):
    f("lin", *F, "p.lda=%d" % lda)
for a, b in PAIRS + [(8, 0), (16, 8), (-16, 0), (16, -16), (32, 32), (32, 16), (48, 64)]:
    f("lin", *F, "seg1=%d" % a, "seg2=%d" % b)
    f("lin", *F, "M=256", "seg1=%d" % a, "seg2=%d" % b)
for form in ("lin", "res"):
    for m in ("p.W_s1=0", "p.w_scale_s1=0", "p.bias_s1=0", "p.gamma_s1=0", "p.W_s2=0", "p.w_scale_s2=0", "p.bias_s2=0", "p.gamma_s2=0"):
        f(form, *F, "seg1=16", m)
        f(form, *F, "seg1=16", "seg2=32", m)
f("res", *F)
for m in ("p.gamma=0", "p.res32=0", "p.out32=0", "p.bias=0"):
    f("res", *F, m)
FLN = ("N=256", "ln=1", "ln8=1")
f("res", *FLN)
f("res", "N=256", "ln=1")
f("res", "N=256", "p.out8=1")                         # out8 alone selects the fused form: its weights are missing
for n in (512, 768, 1024):
    f("res", "N=%d" % n, "ln=1", "ln8=1")
for k in (128, 256, 384):
    f("res", *FLN, "K=%d" % k)
for m in ("p.ldc=512", "p.ln_w=0", "p.ln_b=0", "p.ln_stats=0", "p.ln_count=0", "p.out8_scale=0", "p.out8_mt=0"):
    f("res", *FLN, m)
for m in ("p.ln_w_s1=0", "p.ln_b_s1=0", "p.ln_w_s2=0", "p.ln_b_s2=0"):
    f("res", *FLN, "seg1=16", m)
    f("res", *FLN, "seg1=16", "seg2=32", m)
f("res", *FLN, "M=129")
f("res", *FLN, "M=129", "p.out8_mt=1")
f("lin", *F, "out8=1")
for m in ("p.out8_scale=0", "p.out8_mt=0", "p.bias=0"):
    f("lin", *F, "out8=1", m)
f("lin", *F, "out8=1", "M=129", "p.out8_mt=1")
for m in ("p.out16=0", "p.out32=1", "p.res32=1", "p.bias=0", "p.out16_border=1"):
    f("lin", *F, m)
f("lin", "N=128", "p.out16=0")                        # (refused on its shape, with the shape's message, before the output form)

# ---- admit_quantize_fp8, admit_attention ------------------------------------------------------------------
for rows, k, wl in [(64, 128, 0), (64, 64, 0), (0, 128, 0), (1, 128, 0), (32, 128, 1), (64, 128, 1), (64, 192, 1), (64, 256, 1)]:
    CASES.append("q %d %d %d" % (rows, k, wl))
for a in [(2, 1, 1, 0, 0, 0), (2, 577, 1, 0, 0, 0), (0, 577, 1, 0, 0, 0), (2, 0, 1, 0, 0, 0), (2, 577, 0, 0, 0, 0), (-1, 1, 1, 0, 0, 0),
          (2, 577, 2, 1, 1, 10), (2, 577, 2, 1, 0, 10), (2, 577, 2, 1, 1, 0), (2, 577, 3, 1, 1, 10), (2, 577, 3, 0, 0, 0), (2, 1, 1, 1, 1, 1),
          (1 << 20, 1, 1023, 0, 0, 0), (1 << 20, 1, 1024, 0, 0, 0), (1 << 20, 128, 1023, 0, 0, 0), (1 << 20, 129, 512, 0, 0, 0),
          (1 << 20, 129, 511, 0, 0, 0), (1 << 20, 577, 204, 0, 0, 0), (1 << 20, 577, 205, 0, 0, 0)]:
    CASES.append("a %d %d %d %d %d %d" % a)

# ---- the GEMM, convolution and ConvTranspose entries -------------------------------------------------------
for k, s in [(1, 1), (3, 2), (2, 1), (0, 1), (3, 3), (3, 0), (1, 2)]:
    o("conv2d", k, s)
HF = [1, 8, 8, 64, 32]
o("head_final", *HF)
for i, vals in enumerate([(0,), (0,), (0,), (32, 0, 128), (0, 4, 30, 36, -4)]):
    for v in vals:
        o("head_final", *(HF[:i] + [v] + HF[i + 1:]))
C2 = [1, 8, 8, 64, 64, 3, 1, 1, 1, 0]                 # B H W Cin Cout k stride out16 out16_parts act
o("conv2d_forms", *C2)
for i, vals in enumerate([(0,), (0,), (0,), (0, 32), (0, 4), (1, 2), (2, 3, 0), (0,), (0, 2, 3, 4), (1, 2, 3, -1)]):
    for v in vals:
        o("conv2d_forms", *(C2[:i] + [v] + C2[i + 1:]))
o("conv2d_forms", 1, 7, 8, 64, 64, 3, 2, 1, 1, 0)
o("conv2d_forms", 1, 8, 7, 64, 64, 3, 2, 1, 1, 0)
o("conv2d_forms", 1, 8, 8, 64, 64, 3, 1, 0, 2, 0)
o("conv2d_forms", 1, 8, 8, 64, 64, 3, 1, 0, 3, 0)
CT = [1, 8, 8, 64, 0, 8, 1, 0, 0, 0, 0]               # B H W Cin a_wrap Cout out16 act16 out_split pixel_stride lo_off
o("convt_forms", *CT)
for i, vals in enumerate([(0,), (0,), (0,), (0,), (), (0, 4, 6, 12, 16), (0,), (1, 2, 3), (1,), (-8, 4, 8, 12, 16), (8,)]):
    for v in vals:
        o("convt_forms", *(CT[:i] + [v] + CT[i + 1:]))
for out16, split, ps, lo in [(0, 1, 0, 0), (0, 0, 16, 0), (0, 0, 0, 8), (1, 1, 0, 0), (1, 1, 0, 8), (1, 1, 0, 16), (1, 1, 0, 4), (1, 1, 0, 12),
                             (1, 1, 8, 0), (1, 1, 16, 0), (1, 1, 16, 8), (1, 1, 24, 16), (1, 1, 16, 16), (1, 0, 8, 0)]:
    o("convt_forms", 1, 8, 8, 64, 0, 8, out16, 0, split, ps, lo)
for cout, split, ps, lo in [(12, 1, 0, 0), (12, 1, 32, 16), (12, 1, 24, 16), (12, 0, 16, 0), (12, 0, 8, 0), (16, 1, 0, 8), (16, 0, 8, 0), (4, 1, 0, 0),
                            (4, 1, 16, 8)]:
    o("convt_forms", 1, 8, 8, 64, 0, cout, 1, 0, split, ps, lo)
for cin, wrap in [(128, 0), (128, 64), (128, 32), (128, 128), (128, -64), (192, 64), (192, 128), (64, 64), (256, 128), (256, 192)]:
    o("convt_forms", 1, 8, 8, cin, wrap, 8, 1, 0, 0, 0, 0)
CP = [1, 8, 8, 8, 64, 128, 0, 0, 0]                   # B H W Cout Cin_a Cin_b a_wrap_b act16 grid_cap
o("convt_pair", *CP)
for i, vals in enumerate([(0,), (0,), (0,), (0, 4, 12, 16), (0,), (0,), (64, 32, 128, -64), (1, 2, 3), (-8, 8)]):
    for v in vals:
        o("convt_pair", *(CP[:i] + [v] + CP[i + 1:]))
o("convt_pair", 1, 8, 8, 8, 64, 192, 64, 0, 0)
o("convt_pair", 1, 8, 8, 8, 64, 192, 128, 0, 0)
for w, p, c in [(2, 64, 64), (0, 64, 64), (2, 0, 64), (2, 64, 0), (1 << 15, 1 << 15, 64), (1 << 15, (1 << 15) - 1, 64)]:
    o("patch_embed", w, p, c)

# ---- the row-segmented entries ------------------------------------------------------------------------------
for a, b in PAIRS:
    o("linear_segments", M, a, b, 0, 0, 1)
    o("lrl", M, 256, a, b, 0, 0, 0, 0, 0)
    o("layernorm_segments", 0, 0, a, b, 0, M, 256)
    o("attention_segments", 0, 1, 1, 1, M, a, b, 0, 0)
for a, b in [(0, 0), (16, 0), (16, 24)]:
    for bit in (1, 2, 4):
        o("linear_segments", M, a, b, bit, 0, 0)      # each segment's weight null in turn
        o("linear_segments", M, a, b, 0, bit, 1)      # ... and its gamma, in the residual form
        o("linear_segments", M, a, b, 0, bit, 0)
        for arr in range(5):                          # W16, bias, gamma, ln_w, ln_b
            o("lrl", M, 256, a, b, *[bit if i == arr else 0 for i in range(5)])
        for arr in range(6):                          # W8, w_scale, bias, gamma, ln_w, ln_b
            o("fp8_rl_weights", a, b, *[bit if i == arr else 0 for i in range(6)])
        o("layernorm_segments", bit, 0, a, b, 0, M, 256)
        o("layernorm_segments", 0, bit, a, b, 0, M, 256)
    o("linear_segments", M, a, b, 0, 8, 1)            # the residual form without a gamma array
    o("linear_segments", M, a, b, 0, 8, 0)
    o("fp8_rl_weights", a, b, 0, 0, 0, 0, 0, 0)
for n in (4, 6, 128, 256, 512, 768, 1024):
    o("lrl", M, n, 0, 0, 0, 0, 0, 0, 0)
    o("lrl_fp8", M, n, 16, 24, 0, 0, 0, 0, 0)
o("lrl_fp8", M, 256, 24, 16, 0, 0, 0, 0, 0)
o("lrl_fp8", M, 256, 16, 24, 0, 0, 0, 2, 0)
for dim in (0, 64, 128, 192, 256, 512, 768, 1024):
    for y8 in (0, 1):
        o("layernorm_segments", 0, 0, 0, 0, y8, M, dim)
o("layernorm_segments", 0, 0, 0, 0, 0, 0, 256)
o("layernorm_segments", 0, 0, 0, 0, 0, -1, 256)
# attention: out8 windows tokens heads rows_total seg1 seg2 win0 win1
for a in [(1, 2, 8, 3, 16, 0, 0, 0, 0), (1, 2, 8, 2, 16, 0, 0, 0, 0), (0, 2, 8, 3, 16, 0, 0, 0, 0), (0, 0, 8, 2, 16, 0, 0, 0, 0), (0, 2, 0, 2, 16, 0, 0, 0, 0),
          (0, 2, 8, 0, 16, 0, 0, 0, 0), (0, 2, 8, 2, 0, 0, 0, 0, 0), (0, 2, 8, 2, 16, 0, 0, -1, 0), (0, 2, 8, 2, 16, 0, 0, 0, -1),
          # one segment: the windows end inside the rows
          (0, 2, 8, 2, 16, 0, 0, 0, 0), (0, 2, 8, 2, 15, 0, 0, 0, 0), (0, 2, 1, 2, 2, 0, 0, 0, 0), (0, 2, 1, 2, 1, 0, 0, 0, 0),
          (0, 2, 577, 2, 1154, 0, 0, 0, 0), (0, 2, 577, 2, 1153, 0, 0, 0, 0),
          # two segments
          (0, 4, 8, 2, 32, 16, 0, 2, 2), (0, 4, 8, 2, 32, 15, 0, 2, 2), (0, 5, 8, 2, 40, 16, 0, 2, 2), (0, 3, 8, 2, 32, 16, 0, 2, 2),
          (0, 4, 8, 2, 31, 16, 0, 2, 2), (0, 4, 8, 2, 33, 17, 0, 2, 2), (0, 2, 577, 2, 1154 + 3, 580, 0, 1, 1), (0, 2, 577, 2, 1154 + 2, 580, 0, 1, 1),
          (0, 2, 577, 2, 1154 + 3, 576, 0, 1, 1),
          # three segments
          (0, 6, 8, 2, 48, 16, 32, 2, 2), (0, 6, 8, 2, 48, 15, 32, 2, 2), (0, 6, 8, 2, 47, 16, 31, 2, 2), (0, 3, 8, 2, 48, 16, 32, 2, 2),
          (0, 4, 8, 2, 48, 16, 32, 2, 2), (0, 6, 8, 2, 47, 16, 32, 2, 2), (0, 7, 8, 2, 48, 16, 32, 2, 2), (0, 6, 8, 2, 50, 17, 34, 2, 2),
          (0, 3, 577, 2, 1740, 580, 1160, 1, 1), (0, 3, 577, 2, 1739, 580, 1160, 1, 1), (0, 3, 577, 2, 1737, 580, 1156, 1, 1),
          (1, 6, 8, 2, 48, 16, 32, 2, 2), (1, 6, 8, 1, 48, 16, 32, 2, 2)]:
    o("attention_segments", *a)

# ---- the layout entries ---------------------------------------------------------------------------------------
GRIDS = (0, 4, 8, 12, 64, 72)
for m in [(1, 8, 8, 64), (0, 8, 8, 64), (65535, 8, 8, 64), (65536, 8, 8, 64), (1, 0, 8, 64), (1, 8, 0, 64), (1, 8, 8, 0), (1, 65536, 32768, 64),
          (1, 65536, 32767, 64), (1, 8, 8, 65535 * 32), (1, 8, 8, 65535 * 32 + 1)]:
    o("map", *m)
for b in [(3, 8, 16), (0, 8, 16), (3, 0, 16), (3, 8, 0), (3, 32768, 16), (3, 32769, 16), (3, 8, 32768), (3, 8, 32769)]:
    o("bilinear", *b)
for grid in GRIDS:
    o("patchify", 1, grid)
    o("patchify_windows", 35, grid)
    o("merge", 1, 35, 0, 5, 0, grid, 64)
    o("fov_add", 1, grid, 64, grid * grid + 1)
    o("fov_add", 1, grid, 64, grid * grid)
for batch in (0, 1024, 1025):
    o("patchify", batch, 8)
for windows in (0, 35 * 1024, 35 * 1024 + 1):
    o("patchify_windows", windows, 8)
for c in [(2, 65, 64), (0, 65, 64), (2, 0, 64), (2, 65, 0)]:
    o("cls_rows", *c)
MG = [1, 35, 0, 5, 3, 8, 64]                          # batch wpi win0 steps padding grid dim
o("merge", *MG)
for i, vals in enumerate([(0,), (0, 24, 25), (-1, 10, 11), (0, 1, 5, 6), (-1, 0, 4), (), (0,)]):
    for v in vals:
        o("merge", *(MG[:i] + [v] + MG[i + 1:]))
for steps, padding, grid in [(1, 0, 8), (1, 1, 8), (2, 1, 8), (5, 31, 64), (5, 32, 64), (5, 5, 12), (3, 3, 8), (3, 4, 8)]:
    o("merge", 1, 35, 0, steps, padding, grid, 64)
for c in [(64, 64, 64), (0, 64, 64), (64, 0, 64), (64, 64, 0), (1 << 40, 64, 64)]:
    o("concat_channels", *c)
for a in [(0, 8, 64, 65), (1, 8, 0, 65), (1, 8, 64, 0), (1, 8, 64, 577)]:
    o("fov_add", *a)
for a in [(1, 8, 64), (0, 8, 64), (1, 0, 64), (1, 8, 0), (1, 32768, 2), (1, 32768, 1), (1, 46340, 1), (1, 46341, 1)]:
    o("fov_final", *a)

assert len(set(CASES)) > 0.9 * len(CASES)


def case_list_digest():
    import hashlib
    return hashlib.sha256("\n".join(CASES).encode()).hexdigest()


def table():
    """(digest of the case list the answers are for, the answers in the order of CASES): one answer to a line, `0` or
    `<code>\\t<message>`"""
    digest, answers = None, []
    for ln in open(os.path.join(GOLDEN, "admission_table.txt")):
        if ln.startswith("# cases "):
            digest = ln.split()[2]
        elif not ln.startswith("#"):
            answers.append(ln.rstrip("\n"))
    return digest, answers
