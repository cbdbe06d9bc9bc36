"""Kernel-level tests (-m gpu) of the split-operand forms of the GEMM / conv / ConvTranspose epilogues (gemm_core.h
store_16bit_lo, GemmParams::ldc16 / lo_off16 / hi2_off16) through me_op_conv2d_forms, me_op_linear_split and
me_op_conv_transpose2x2_forms, which build GemmParams with the code pipeline.hip's conv / linear / convt helpers use
(csrc/gemm_params.h).

A split value is the pair hi = T(v), lo = T(v - hi).  On the INPUT side the kernel only sees K (or Cin) doubled or
tripled against weights that repeat themselves (weights.hip); the tests build those operands.  Every check is one of
  * fp64: the conv / matmul / conv-transpose of hi.double() + lo.double() with the 16-bit weights: only f32 accumulation
    differs, so the unsplit tests' bounds hold (max_abs_rel 3e-5 conv, 2e-5 linear / ConvT: the lo products are 2^-11
    smaller than the hi ones); a split 16-bit result is compared as hi + lo with the representation term of
    layout_refs.SPLIT_REL on top (2^-22 f16, 2^-16 bf16, relative to the element).  A dropped or misplaced lo costs up to
    2^-12 relative;
  * structure, whatever the evaluation order: |lo| <= ulp(hi) / 2, the second hi of [hi | lo | hi] equals the first,
    ReLU leaves hi >= 0 and lo == 0 where hi == 0, borders / guards / foreign channels keep their sentinel;
  * bit for bit: the same problem through other tiles, through the run-time mode 0 of the epilogue, and against the
    launch's own f32 output (hi == T(act(out32)), lo == T(act(out32) - hi)).

Compiled-in epilogue combinations of gemm_core.h's dispatch, and the case here (or elsewhere) that launches each:
  EPI_STORE
    mode 1  (16-bit only, bias, no activation)     test_conv_forms_against_fp64[plain16]; test_gpu_ops test_linear_scaled_cols
    mode 2  (... + GELU: fc1)                      test_gpu_ops.py test_linear_gelu           (no convolution uses it)
    mode 3  (fp8 output)                           test_gpu_fp8.py                            (the fp8 GEMM only)
    Out16|Border                                   [b16]
    Out32|Out16|Border                             [o32_b16]            (and every test_gpu_ops.py convolution without residuals)
    Res|Out32|Out16|Border                         [res_o32_b16]
    Res|ResB|Out32|Out16|Border                    [res2_o32_b16]       (and test_gpu_ops.py's residual convolutions)
    Out16|Border|TapBias                           test_gpu_pipeline.py test_composed_features_equal_the_two_layers (out of scope)
    Res|Out16|Border                               [res_b16]
    Res|Out16|Lo|Hi2                               [res_triple]         (the fusion blocks' resnet2 under SPLIT_FUSION_OUT, fused)
    Res|Out16|Lo                                   [res_split]          (... not fused)
    Out16                                          [relu16]
    Out16|Lo                                       [split], [head0_split] (the head's first convolution under SPLIT_HEAD)
    mode 0  (everything else, checked at run time) [b_split] (Out16|Lo|Border: the fuse 1x1), [o32_split], [o32_b_triple],
                                                   [res2_split], every case again with bias = NULL, me_op_linear_split
  EPI_CONVT
    mode 4  (16-bit)          test_convt_forms[plain16], [slice]
    mode 5  (f32)             test_convt_forms[f32]
    mode 6  (both)            test_convt_forms[both]        (and test_gpu_ops.py test_conv_transpose)
    mode 7  (16-bit [hi|lo])  test_convt_forms[split], [cat_slice_0], [cat_slice_1]
    mode 0                    test_convt_forms[relu_split], [both_split]
The 352-row tile (tile_cfg 10) carries none of the compiled-in modes (it serves qkv / fc1 through modes 1 and 2)."""
import math
import random

import pytest
import torch
import torch.nn.functional as F

import layout_refs as R
from util import TORCH16, ctx_for, pack_conv, pack_convt, ptr

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SENT = -7.5
GUARD = 4096
CONV_BOUND, LIN_BOUND = 3e-5, 2e-5       # max |err| / rms(ref) of an f32 result: the bounds of test_gpu_ops.py's unsplit tests


def call(ctx, fn, *args):
    """One launch on the context's stream, fenced on both sides: the buffers were filled on torch's stream."""
    torch.cuda.synchronize()
    ctx._check(fn(ctx.handle, *args))
    ctx.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, want, zero_sign=True):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    eq = bits(got) == bits(want)
    if not zero_sign:
        eq |= (got == 0) & (want == 0)
    if not bool(eq.all()):
        i = tuple((~eq).nonzero()[0].tolist())
        raise AssertionError(f"{int((~eq).sum())} of {eq.numel()} elements differ; first at {i}: {got[i].item()!r} != {want[i].item()!r}")


def sent_buf(numel, dt):
    buf = torch.full((numel + GUARD,), SENT, dtype=dt, device="cuda")
    return buf


def split_operand(v, T, copies):
    """[..][C] f32 -> the operand as stored: 1: T(v); 2: [hi | lo]; 3: [hi | lo | hi]."""
    hi, lo = R.split_hi_lo(v, T)
    return {1: hi, 2: torch.cat([hi, lo], -1), 3: torch.cat([hi, lo, hi], -1)}[copies]


def check_16bit(px, ref, T, parts, bound, relu, out32=None, tag=""):
    """px [M][parts * N]: the 16-bit output pixels; ref [M][N] f64: the activated fp64 result; out32: the launch's own
    f32 output [M][N] where it wrote one."""
    px = px.cpu()
    M, N = ref.shape
    hi = px[:, :N]
    rms = float(ref.pow(2).mean().sqrt().clamp_min(1e-30))
    floor = 2.0 ** -25 if T == torch.float16 else 0.0               # the f16 subnormal grid
    fin = torch.isfinite(hi)
    assert bool(fin.all()), tag
    if parts == 1:
        # out16 = T(v32), |v32 - ref| <= bound * rms, one rounding of v32
        tol = bound * rms + R.EPS16[T] * (ref.abs() + bound * rms) + floor
        err = (hi.double() - ref).abs()
    else:
        lo = px[:, N:2 * N]
        assert bool((lo.double().abs() <= R.ulp16(hi) / 2).all()), f"{tag}: |lo| > ulp(hi) / 2"
        tol = bound * rms + R.SPLIT_REL[T] * (ref.abs() + bound * rms) + floor
        err = (hi.double() + lo.double() - ref).abs()
        if relu:
            assert bool((lo[hi == 0] == 0).all()), f"{tag}: lo != 0 under a zero hi"
        if parts == 3:
            same_bits(px[:, 2 * N:], hi)
    worst = float((err / tol).max())
    print(f"{tag} parts {parts}: worst error / bound {worst:.3f} (max_abs_rel {float(err.max()) / rms:.2e})")
    assert worst <= 1.0, tag
    if relu:
        assert bool((hi >= 0).all()), tag
    if out32 is not None:
        a = out32.cpu().float()
        a = a.clamp_min(0.0) if relu else a
        whi, wlo = R.split_hi_lo(a, T)
        same_bits(hi, whi, zero_sign=not relu)
        if parts >= 2:
            same_bits(px[:, N:2 * N], wlo, zero_sign=False)


# ---------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------
def conv_problem(T, B, H, W, Cin, Cout, k, stride, copies, seed, res=0, bias=True, scale=1.0):
    """Operands of one convolution: v f32 NCHW, given to the kernel as zero-bordered NHWC pixels of `copies` parts against
    weights that repeat themselves per tap (copies 3: [W | W | W2], as a composed layer has them); fp64 reference of the
    pre-activation result [M][Cout] with the residuals added."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, Cin, H, W, generator=g) * scale
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).to(T)
    w2 = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).to(T)
    b = torch.randn(Cout, generator=g) if bias else None
    op = split_operand(R.nchw_to_nhwc(v), T, copies)                              # [B][H][W][copies * Cin]
    xb = torch.zeros(B, H + 2, W + 2, copies * Cin, dtype=T)
    xb[:, 1:-1, 1:-1] = op
    wp = pack_conv(w.float()).reshape(Cout, k * k, Cin)
    parts_w = {1: [wp], 2: [wp, wp], 3: [wp, wp, pack_conv(w2.float()).reshape(Cout, k * k, Cin)]}[copies]
    wd = torch.cat(parts_w, dim=2).reshape(Cout, -1).to(T)
    hi = op[..., :Cin].double()
    val = hi + op[..., Cin:2 * Cin].double() if copies > 1 else hi
    pad = (k - 1) // 2
    ref = F.conv2d(R.nhwc_to_nchw(val), w.double(), b.double() if bias else None, stride=stride, padding=pad)
    if copies == 3:
        ref = ref + F.conv2d(R.nhwc_to_nchw(hi), w2.double(), None, stride=stride, padding=pad)
    Ho, Wo = H // stride, W // stride
    ref = R.nchw_to_nhwc(ref).reshape(B * Ho * Wo, Cout)
    rs = [torch.randn(B * Ho * Wo, Cout, generator=g) for _ in range(res)]
    for r in rs:
        ref = ref + r.double()
    return dict(xb=xb.cuda(), w=wd.cuda(), bias=b.cuda() if bias else None, res=[r.cuda() for r in rs], ref=ref,
                shape=(B, H, W, copies * Cin, Cout, k, stride), Ho=Ho, Wo=Wo)


def run_conv(ctx, T, pr, parts, border, out32, act, act_both, cfg, bias="own"):
    """One launch; returns (interior 16-bit pixels [M][parts * Cout] or None, out32 [M][Cout] or None) after checking
    that border, guard and (when not asked for) the other output keep the sentinel."""
    B, H, W, Cin, Cout, k, stride = pr["shape"]
    Ho, Wo = pr["Ho"], pr["Wo"]
    M = B * Ho * Wo
    bd = 1 if border else 0
    n16 = B * (Ho + 2 * bd) * (Wo + 2 * bd) * parts * Cout
    b16 = sent_buf(n16, T) if parts else None
    b32 = sent_buf(M * Cout, torch.float32)
    res = pr["res"] + [None, None]
    bias_t = pr["bias"] if bias == "own" else bias
    call(ctx, ctx.lib.me_op_conv2d_forms, ptr(pr["xb"]), B, H, W, Cin, ptr(pr["w"]), Cout, k, stride, ptr(bias_t), ptr(res[0]),
         ptr(res[1]), ptr(b32) if out32 else None, ptr(b16), bd, max(parts, 1), act, act_both, cfg)
    o32 = None
    if out32:
        o32 = b32[:M * Cout].reshape(M, Cout)
    else:
        assert bool((b32 == SENT).all())
    assert bool((b32[M * Cout:] == SENT).all())
    px = None
    if parts:
        assert bool((b16[n16:] == SENT).all()), "wrote behind the 16-bit output"
        img = b16[:n16].reshape(B, Ho + 2 * bd, Wo + 2 * bd, parts * Cout)
        if bd:
            edge = torch.ones(B, Ho + 2, Wo + 2, dtype=torch.bool, device="cuda")
            edge[:, 1:-1, 1:-1] = False
            assert bool((img[edge] == SENT).all()), "the border was written"
            img = img[:, 1:-1, 1:-1]
        px = img.reshape(M, parts * Cout)
    return px, o32


# name -> (parts, border, out32, residuals, act, act_both); act 2 = ReLU
CONV_FORMS = {
    "plain16": (1, 0, 0, 0, 0, 0), "relu16": (1, 0, 0, 0, 2, 0), "b16": (1, 1, 0, 0, 2, 0), "o32_b16": (1, 1, 1, 0, 2, 0),
    "res_o32_b16": (1, 1, 1, 1, 2, 0), "res2_o32_b16": (1, 1, 1, 2, 2, 1), "res_b16": (1, 1, 0, 1, 0, 0),
    "res_triple": (3, 0, 0, 1, 0, 0), "res_split": (2, 0, 0, 1, 0, 0), "split": (2, 0, 0, 0, 2, 0),
    "b_split": (2, 1, 0, 0, 0, 0), "o32_split": (2, 0, 1, 0, 2, 0), "o32_b_triple": (3, 1, 1, 1, 2, 1),
    "res2_split": (2, 1, 1, 2, 0, 0), "f32_only": (0, 0, 1, 0, 2, 1),
}


def conv_form_case(ctx, dtype, form, geom, copies, cfgs, seed, bound=CONV_BOUND):
    T = TORCH16[dtype]
    parts, border, out32, nres, act, act_both = CONV_FORMS[form]
    B, H, W, Cin, Cout, k, stride = geom
    pr = conv_problem(T, B, H, W, Cin, Cout, k, stride, copies, seed, res=nres)
    relu = act == 2
    ref16 = pr["ref"].clamp_min(0.0) if relu else pr["ref"]
    ref32 = ref16 if (relu and act_both) else pr["ref"]
    first = None
    ctx.status_flags()
    for cfg in cfgs:
        tag = f"{form} {dtype} {geom} x{copies} cfg {cfg}"
        px, o32 = run_conv(ctx, T, pr, parts, border, out32, act, act_both, cfg)
        if o32 is not None:
            rms = float(ref32.pow(2).mean().sqrt())
            e32 = float((o32.double().cpu() - ref32).abs().max()) / rms
            print(f"{tag}: out32 max_abs_rel {e32:.2e}")
            assert e32 < bound, tag
        if parts:
            check_16bit(px, ref16, T, parts, bound, relu, o32, tag)
        if first is None:
            first = (px, o32)
        else:   # every convolution tile walks K in the same order (gemm_core.h SlabWalk): the tile changes no bit
            if parts:
                same_bits(px, first[0])
            if o32 is not None:
                same_bits(o32, first[1])
    assert ctx.status_flags() == 0
    return pr, first


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", sorted(CONV_FORMS))
def test_conv_forms_against_fp64(dtype, form):
    """Every output form on a 3x3 convolution with doubled Cin, ragged M (B * H * W = 2 * 13 * 11), Cout = 132 (not a
    multiple of 8: the last granule of a row is the half-granule store, and lo_off16 = 132 is off the 16-byte grid), the
    automatic tile and tile 0 bit for bit; then on a stride-2 1x1 with tripled Cin."""
    ctx = ctx_for("tiny", dtype)
    conv_form_case(ctx, dtype, form, (2, 13, 11, 64, 132, 3, 1), 2, (-1, 0, 2), 11)
    conv_form_case(ctx, dtype, form, (1, 12, 20, 64, 40, 1, 2), 3, (-1, 1), 12)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", sorted(set(CONV_FORMS) - {"f32_only"}))
def test_compiled_in_modes_equal_the_run_time_mode(dtype, form):
    """gemm_core.h picks a compiled-in option combination only when the launch has a bias (cf_ok); without one the same
    launch runs mode 0, every option checked per granule at run time.  A NULL bias and a bias of zeros add the same
    +0.0 to every accumulator (EpiLane::bias is zero-initialised and always added), so the two must agree bit for bit."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    parts, border, out32, nres, act, act_both = CONV_FORMS[form]
    pr = conv_problem(T, 2, 17, 9, 128, 72, 3, 1, 2, 21, res=nres, bias=False)
    zeros = torch.zeros(72, device="cuda")
    a = run_conv(ctx, T, pr, parts, border, out32, act, act_both, 0, bias=None)
    b = run_conv(ctx, T, pr, parts, border, out32, act, act_both, 0, bias=zeros)
    same_bits(a[0], b[0])
    if out32:
        same_bits(a[1], b[1])
    check_16bit(a[0], pr["ref"].clamp_min(0.0) if act else pr["ref"], T, parts, CONV_BOUND, act == 2, a[1], form)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,geom", [
    ("split", (1, 48, 32, 256, 128, 3, 1)),          # head0_split: the head's first convolution, Cin = 2 * 256 -> 128; tiles -1, 0, 12
    ("res_triple", (1, 48, 32, 64, 256, 3, 1)),      # resnet2's second convolution under SPLIT_FUSION_OUT; tiles -1, 0, 9, 11
    ("b_split", (2, 16, 16, 32, 256, 3, 1)),         # tiles -1, 0, 9
    ("o32_b16", (1, 48, 48, 128, 256, 3, 1)),        # the decoder's convs[i] with a split input (SPLIT_DEC_CONVS)
])
def test_halo_tiles_with_doubled_cin(dtype, form, geom):
    """The "same K order" property of test_gpu_ops.py test_conv3x3_halo_tile for doubled Cin and the split outputs: the
    automatic tile, tile 0 and the halo tiles the launch admits (9: 16 x 16 pixels x 256 channels; 11: 12 x 16 pixels; 12:
    128 channels) give identical hi and lo."""
    ctx = ctx_for("tiny", dtype)
    B, H, W, Cin, Cout, k, s = geom
    cfgs = [-1, 0]
    if Cout % 256 == 0:
        cfgs.append(9)
        if H % 12 == 0:
            cfgs.append(11)
    if Cout % 128 == 0:
        cfgs.append(12)
    conv_form_case(ctx, dtype, form, geom, 2, cfgs, 31)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fuse_1x1_at_the_models_k(dtype):
    """encoder.rs:323-325 fuse_lowres under split operands: a 1x1 convolution over pixels of [hi(2 e3) | lo(2 e3)], K = 2 * 2 *
    1024, into a zero-bordered [hi | lo] map (Out16|Lo|Border: run-time mode 0)."""
    ctx = ctx_for("tiny", dtype)
    conv_form_case(ctx, dtype, "b_split", (1, 12, 10, 2048, 1024, 1, 1), 2, (-1, 0), 41)


def test_conv_forms_random_shapes():
    """30 seeded random convolutions in the manner of test_gpu_ops.py test_conv2d_random_shapes: odd maps, 1x1 and 3x3,
    stride 1 and 2, any implicit-GEMM tile, any output form, input parts 1 / 2 / 3, both types."""
    rnd = random.Random(4242)
    forms = sorted(CONV_FORMS)
    for it in range(30):
        dtype = rnd.choice(DTYPES)
        k, s = rnd.choice([1, 3, 3]), rnd.choice([1, 1, 2])
        B = rnd.choice([1, 1, 2, 3])
        H, W = (2 * rnd.randrange(1, 12), 2 * rnd.randrange(1, 12)) if s == 2 else (rnd.randrange(1, 23), rnd.randrange(1, 23))
        copies = rnd.choice([1, 2, 2, 3])
        Cin = 64 * rnd.choice([1, 2, 3]) if copies != 2 else 32 * rnd.choice([1, 2, 3, 4])
        Cout = 4 * rnd.choice([1, 2, 8, 9, 16, 33, 64])
        cfg = rnd.choice([-1, 0, 1, 2, 3, 4, 5, 7, 8])
        form = rnd.choice(forms)
        conv_form_case(ctx_for("tiny", dtype), dtype, form, (B, H, W, Cin, Cout, k, s), copies, (cfg,), 5000 + it)


# ---------------------------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------------------------
def linear_split_case(ctx, dtype, M, N, K, copies, cfg, act, with32, seed):
    T = TORCH16[dtype]
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(M, K, generator=g)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(T)
    bias = torch.randn(N, generator=g)
    A = split_operand(v, T, copies).cuda()
    Wd = torch.cat([w] * copies, dim=1).cuda()
    val = A[:, :K].double() + (A[:, K:2 * K].double() if copies > 1 else 0.0)
    ref = val @ w.cuda().double().T + bias.cuda().double()
    if copies == 3:
        ref = ref + A[:, :K].double() @ w.cuda().double().T
    ref = ref.cpu()
    ref16 = ref.clamp_min(0.0) if act == 2 else ref
    b16, b32 = sent_buf(M * 2 * N, T), sent_buf(M * N, torch.float32)
    bd = bias.cuda()
    ctx.status_flags()
    call(ctx, ctx.lib.me_op_linear_split, M, N, copies * K, ptr(A), ptr(Wd), ptr(bd), ptr(b16), ptr(b32) if with32 else None, act, cfg)
    assert ctx.status_flags() == 0
    assert bool((b16[M * 2 * N:] == SENT).all()) and bool((b32[M * N:] == SENT).all())
    tag = f"linear_split {dtype} {M}x{N}x{K} x{copies} cfg {cfg} act {act}"
    o32 = None
    if with32:
        o32 = b32[:M * N].reshape(M, N)
        rms = float(ref16.pow(2).mean().sqrt())
        e32 = float((o32.double().cpu() - ref16).abs().max()) / rms        # (as me_op_linear: the activation applies to both outputs)
        print(f"{tag}: out32 max_abs_rel {e32:.2e}")
        assert e32 < LIN_BOUND, tag
    else:
        assert bool((b32 == SENT).all())
    px = b16[:M * 2 * N].reshape(M, 2 * N)
    check_16bit(px, ref16, T, 2, LIN_BOUND, act == 2, o32, tag)
    return px


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,copies,cfg", [(577, 256, 128, 2, -1), (1000, 132, 192, 2, 0), (2309, 384, 128, 3, 1), (333, 64, 256, 1, 4),
                                              (705, 256, 256, 2, 10)])
def test_linear_split(dtype, M, N, K, copies, cfg):
    """me_op_linear_split: [hi | lo] rows of 2 N, with and without the f32 copy and the ReLU; tile 10 is the 352-row tile,
    which has no compiled-in mode."""
    ctx = ctx_for("tiny", dtype)
    a = linear_split_case(ctx, dtype, M, N, K, copies, cfg, 0, True, M + N)
    b = linear_split_case(ctx, dtype, M, N, K, copies, cfg, 0, False, M + N)
    same_bits(a, b)                                     # Out32|Out16|Lo and Out16|Lo: the f32 copy changes no 16-bit bit
    linear_split_case(ctx, dtype, M, N, K, copies, cfg, 2, True, M + N + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_split_more_tiles_than_workgroups(dtype):
    """Ragged M, N = 132 (not a multiple of 8: the half-granule store, for hi and for lo) and 1094 x 3 tiles of 64 x 64 rows --
    several rounds of the persistent grid."""
    ctx = ctx_for("tiny", dtype)
    linear_split_case(ctx, dtype, 70001, 132, 64, 2, 2, 0, True, 9)


# ---------------------------------------------------------------------------------------------------------------
# ConvTranspose 2x2
# ---------------------------------------------------------------------------------------------------------------
# name -> (out32, out16, border, act16, out_split, wide (pixel_stride / Cout, 0: dense), slice offset / Cout, lo_off / Cout)
CONVT_FORMS = {
    "plain16": (0, 1, 1, 0, 0, 0, 0, 0), "f32": (1, 0, 0, 0, 0, 0, 0, 0), "both": (1, 1, 0, 0, 0, 0, 0, 0),
    "split": (0, 1, 1, 0, 1, 0, 0, 0), "slice": (0, 1, 0, 0, 0, 3, 1, 0),
    "cat_slice_0": (0, 1, 0, 0, 1, 4, 0, 2), "cat_slice_1": (0, 1, 0, 0, 1, 4, 1, 2),     # enc.cat: [up2 hi | lowres hi | up2 lo | lowres lo]
    "relu_split": (0, 1, 1, 2, 1, 0, 0, 0), "both_split": (1, 1, 0, 0, 1, 0, 0, 0),
}


def convt_case(ctx, dtype, form, geom, copies, cfg, seed, bias=True):
    T = TORCH16[dtype]
    out32, out16, border, act16, out_split, wide, c0, lo_off = CONVT_FORMS[form]
    B, H, W, Cin, Cout = geom
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, H, W, Cin, generator=g)
    w = (torch.randn(Cin, Cout, 2, 2, generator=g) / math.sqrt(Cin)).to(T)
    b = torch.randn(Cout, generator=g) if bias else None
    A = split_operand(v, T, copies).reshape(B * H * W, copies * Cin).cuda()
    Wd = torch.cat([pack_convt(w.float())] * copies, dim=1).to(T).cuda()
    val = A[:, :Cin].double().cpu() + (A[:, Cin:2 * Cin].double().cpu() if copies > 1 else 0.0) + \
        (A[:, :Cin].double().cpu() if copies == 3 else 0.0)
    ref = F.conv_transpose2d(R.nhwc_to_nchw(val.reshape(B, H, W, Cin)), w.double(), b.double() if bias else None, stride=2)
    ref = R.nchw_to_nhwc(ref).reshape(B * 4 * H * W, Cout)
    relu = act16 == 2
    ref16 = ref.clamp_min(0.0) if relu else ref
    stride_px = wide * Cout if wide else (2 * Cout if out_split else Cout)
    lo_at = (lo_off * Cout if lo_off else Cout) if out_split else 0
    oH, oW = 2 * H + 2 * border, 2 * W + 2 * border
    n16 = B * oH * oW * stride_px
    b16, b32 = sent_buf(n16, T), sent_buf(B * 4 * H * W * Cout, torch.float32)
    bd = b.cuda() if bias else None
    ctx.status_flags()
    call(ctx, ctx.lib.me_op_conv_transpose2x2_forms, ptr(A), B, H, W, copies * Cin, ptr(Wd), Cout, ptr(bd),
         ptr(b32) if out32 else None, ptr(b16[c0 * Cout:]) if out16 else None, border, act16, out_split,
         wide * Cout, lo_off * Cout, cfg)
    assert ctx.status_flags() == 0
    tag = f"convt {form} {dtype} {geom} x{copies} cfg {cfg}"
    assert bool((b16[n16:] == SENT).all()) and bool((b32[B * 4 * H * W * Cout:] == SENT).all()), tag
    o32 = None
    if out32:
        o32 = b32[:B * 4 * H * W * Cout].reshape(-1, Cout)
        rms = float(ref.pow(2).mean().sqrt())
        e32 = float((o32.double().cpu() - ref).abs().max()) / rms
        print(f"{tag}: out32 max_abs_rel {e32:.2e}")
        assert e32 < LIN_BOUND, tag
    else:
        assert bool((b32 == SENT).all()), tag
    px = None
    if out16:
        img = b16[:n16].reshape(B, oH, oW, stride_px)
        written = torch.zeros(B, oH, oW, stride_px, dtype=torch.bool, device="cuda")
        inner = written[:, 1:-1, 1:-1] if border else written
        inner[..., c0 * Cout:(c0 + 1) * Cout] = True
        if out_split:
            inner[..., c0 * Cout + lo_at:c0 * Cout + lo_at + Cout] = True
        assert bool((img[~written] == SENT).all()), f"{tag}: wrote outside its channels / into the border"
        core = img[:, 1:-1, 1:-1] if border else img
        hi = core[..., c0 * Cout:(c0 + 1) * Cout].reshape(-1, Cout)
        px = torch.cat([hi, core[..., c0 * Cout + lo_at:c0 * Cout + lo_at + Cout].reshape(-1, Cout)], dim=1) if out_split else hi
        check_16bit(px, ref16, T, 2 if out_split else 1, LIN_BOUND, relu, o32, tag)
    else:
        assert bool((b16 == SENT).all()), tag
    return px, o32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", sorted(CONVT_FORMS))
def test_convt_forms(dtype, form):
    """Every ConvTranspose output form: odd map (2 x 9 x 7 pixels: image and row ends inside a tile), doubled and tripled
    Cin, bordered or dense or a channel slice of a wider map whose other channels keep their sentinel; the automatic
    tile and tiles 0 and 2 bit for bit."""
    ctx = ctx_for("tiny", dtype)
    first = None
    for cfg in (-1, 0, 2):
        got = convt_case(ctx, dtype, form, (2, 9, 7, 64, 40), 2, cfg, 51)
        if first is None:
            first = got
        else:
            for a, b in zip(got, first):
                if a is not None:
                    same_bits(a, b)
    convt_case(ctx, dtype, form, (1, 5, 11, 64, 24), 3, -1, 52, bias=False)
    convt_case(ctx, dtype, form, (3, 16, 16, 128, 128), 1, 1, 53)


@pytest.mark.parametrize("dtype", DTYPES)
def test_convt_modes_agree(dtype):
    """The compiled-in ConvTranspose modes against one another and against the run-time mode 0 on the same tile: the
    [hi | lo] of mode 7 is the [hi | lo] of the launch that also writes f32 (mode 0); mode 6's two outputs are mode 4's and
    mode 5's; mode 7's hi is mode 4's 16-bit output."""
    ctx = ctx_for("tiny", dtype)
    geom = (2, 12, 10, 128, 64)
    r = {f: convt_case(ctx, dtype, f, geom, 2, 0, 61) for f in ("plain16", "f32", "both", "split", "both_split")}
    same_bits(r["split"][0], r["both_split"][0])
    same_bits(r["both"][1], r["f32"][1]), same_bits(r["both"][1], r["both_split"][1])
    same_bits(r["both"][0], r["plain16"][0]), same_bits(r["split"][0][:, :64], r["plain16"][0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_convt_into_the_cat_slices_at_the_models_channels(dtype):
    """encoder.rs:316-320 under split operands: upsample2's last ConvTranspose and upsample_lowres write the two halves of
    `enc.cat`, pixels of [up2 hi | lowres hi | up2 lo | lowres lo] with e3 = 1024 channels each, from split inputs."""
    ctx = ctx_for("tiny", dtype)
    convt_case(ctx, dtype, "cat_slice_0", (1, 8, 8, 512, 1024), 2, -1, 71, bias=False)
    convt_case(ctx, dtype, "cat_slice_1", (1, 8, 8, 1024, 1024), 2, -1, 72)


def test_convt_forms_random_shapes():
    rnd = random.Random(777)
    forms = sorted(CONVT_FORMS)
    for it in range(20):
        dtype = rnd.choice(DTYPES)
        geom = (rnd.choice([1, 2, 3]), rnd.randrange(1, 15), rnd.randrange(1, 15), 64 * rnd.choice([1, 2, 3]), 8 * rnd.choice([1, 3, 8, 16, 33]))
        convt_case(ctx_for("tiny", dtype), dtype, rnd.choice(forms), geom, rnd.choice([1, 2, 3]), rnd.choice([-1, 0, 1, 2, 3, 4]),
                   6000 + it, bias=rnd.random() < 0.7)


# ---------------------------------------------------------------------------------------------------------------
# overflow, argument errors
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv_split", "conv_triple_border", "linear_split", "convt_split"])
def test_overflow_of_a_split_output(kind):
    """A value past 65504 (a bias of 7e4 on one output channel) leaves hi = +inf and lo = 0 and raises
    ME_STATUS_OVERFLOW_16BIT on f16; the same launch on bf16 stays finite and raises nothing."""
    for dtype in DTYPES:
        ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
        ctx.status_flags()
        if kind.startswith("conv_"):
            parts, border = (2, 0) if kind == "conv_split" else (3, 1)
            pr = conv_problem(T, 1, 9, 7, 64, 40, 3, 1, 2, 81)
            pr["bias"][5] = 7.0e4
            px, _ = run_conv(ctx, T, pr, parts, border, 0, 0, 0, -1)
            N = 40
        elif kind == "linear_split":
            M, N, K = 100, 40, 64
            A = split_operand(torch.randn(M, K, generator=torch.Generator().manual_seed(82)), T, 2).cuda()
            Wd = torch.zeros(N, 2 * K, dtype=T, device="cuda")
            bias = torch.zeros(N, device="cuda")
            bias[5] = 7.0e4
            px = torch.full((M, 2 * N), SENT, dtype=T, device="cuda")
            call(ctx, ctx.lib.me_op_linear_split, M, N, 2 * K, ptr(A), ptr(Wd), ptr(bias), ptr(px), None, 0, -1)
        else:
            B, H, W, Cin, N = 1, 5, 6, 64, 40
            A = split_operand(torch.randn(B * H * W, Cin, generator=torch.Generator().manual_seed(83)), T, 2).cuda()
            Wd = torch.zeros(4 * N, 2 * Cin, dtype=T, device="cuda")
            bias = torch.zeros(N, device="cuda")
            bias[5] = 7.0e4
            px = torch.full((B * 4 * H * W, 2 * N), SENT, dtype=T, device="cuda")
            call(ctx, ctx.lib.me_op_conv_transpose2x2_forms, ptr(A), B, H, W, 2 * Cin, ptr(Wd), N, ptr(bias), None, ptr(px), 0, 0, 1, 0, 0, -1)
        flags = ctx.status_flags()
        hi, lo = px[:, :N].float().cpu(), px[:, N:2 * N].float().cpu()
        if dtype == "f16":
            assert flags == 1 and ctx.status_flags() == 0, kind
            assert bool(torch.isinf(hi[:, 5]).all()) and bool((hi[:, 5] > 0).all()) and bool((lo[:, 5] == 0).all()), kind
            keep = [c for c in range(N) if c != 5]
            assert bool(torch.isfinite(hi[:, keep]).all()) and bool(torch.isfinite(lo).all()), kind
            if kind == "conv_triple_border":
                same_bits(px[:, 2 * N:], px[:, :N])
        else:
            assert flags == 0, kind
            assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all()), kind
            assert float((hi[:, 5].double() + lo[:, 5].double() - 7.0e4).abs().max()) < 7.0e4 * 2.0 ** -7, kind


def test_argument_errors_leave_the_context_usable():
    ctx = ctx_for("tiny", "f16")
    lib, h = ctx.lib, ctx.handle
    a = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    w = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    o = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    o32 = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    BAD_ARG, BAD_SHAPE = 1, 2
    cases = [
        (BAD_ARG, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 4, 4, 64, ptr(w), 8, 3, 1, None, None, None, None, ptr(o), 0, 4, 0, 0, -1)),   # parts
        (BAD_ARG, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 4, 4, 64, ptr(w), 8, 3, 1, None, None, None, ptr(o32), None, 0, 2, 0, 0, -1)),  # split without out16
        (BAD_ARG, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 4, 4, 64, ptr(w), 8, 3, 1, None, None, None, None, ptr(o), 0, 2, 1, 0, -1)),   # GELU
        (BAD_SHAPE, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 4, 4, 64, ptr(w), 8, 2, 1, None, None, None, None, ptr(o), 0, 2, 0, 0, -1)),  # k
        (BAD_SHAPE, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 4, 4, 48, ptr(w), 8, 3, 1, None, None, None, None, ptr(o), 0, 2, 0, 0, -1)),  # Cin % 64
        (BAD_SHAPE, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 4, 4, 64, ptr(w), 6, 3, 1, None, None, None, None, ptr(o), 0, 2, 0, 0, -1)),  # Cout % 4
        (BAD_SHAPE, lambda: lib.me_op_conv2d_forms(h, ptr(a), 1, 5, 4, 64, ptr(w), 8, 3, 2, None, None, None, None, ptr(o), 0, 2, 0, 0, -1)),  # odd map, stride 2
        (BAD_ARG, lambda: lib.me_op_linear_split(h, 8, 8, 64, ptr(a), ptr(w), None, None, ptr(o32), 0, -1)),
        (BAD_SHAPE, lambda: lib.me_op_linear_split(h, 8, 8, 72, ptr(a), ptr(w), None, ptr(o), None, 0, -1)),                                  # K % 64
        (BAD_SHAPE, lambda: lib.me_op_linear_split(h, 8, 6, 64, ptr(a), ptr(w), None, ptr(o), None, 0, -1)),                                  # N % 4
        (BAD_SHAPE, lambda: lib.me_op_conv_transpose2x2_forms(h, ptr(a), 1, 2, 2, 64, ptr(w), 12, None, None, ptr(o), 0, 0, 1, 0, 0, -1)),    # Cout % 8
        (BAD_SHAPE, lambda: lib.me_op_conv_transpose2x2_forms(h, ptr(a), 1, 2, 2, 64, ptr(w), 16, None, None, ptr(o), 0, 0, 1, 24, 0, -1)),   # stride < 2 Cout
        (BAD_SHAPE, lambda: lib.me_op_conv_transpose2x2_forms(h, ptr(a), 1, 2, 2, 64, ptr(w), 16, None, None, ptr(o), 0, 0, 1, 64, 8, -1)),   # lo inside hi
        (BAD_ARG, lambda: lib.me_op_conv_transpose2x2_forms(h, ptr(a), 1, 2, 2, 64, ptr(w), 16, None, None, ptr(o), 0, 0, 0, 0, 16, -1)),     # lo_off, no split
        (BAD_ARG, lambda: lib.me_op_conv_transpose2x2_forms(h, ptr(a), 1, 2, 2, 64, ptr(w), 16, None, ptr(o32), None, 0, 0, 1, 0, 0, -1)),    # split, no out16
        (BAD_ARG, lambda: lib.me_op_conv_transpose2x2_forms(h, ptr(a), 1, 2, 2, 64, ptr(w), 16, None, None, ptr(o), 0, 1, 0, 0, 0, -1)),      # GELU
    ]
    for i, (code, launch) in enumerate(cases):
        rc = launch()
        assert rc == code, f"case {i}: returned {rc}, expected {code}: {lib.me_last_error(h)}"
    ctx.synchronize()
    assert bool((o == 0).all()) and bool((o32 == 0).all())          # nothing was launched
    linear_split_case(ctx, "f16", 100, 40, 64, 2, -1, 0, True, 91)   # the context works afterwards
