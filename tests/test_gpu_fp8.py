"""MX block-scaled fp8 path (-m gpu): BASELINE configs[3], ME_DTYPE_FP8.  Kernel-level checks are EXACT in the sense
that matters: the quantisers are compared code for code with a torch restatement of the OCP MX rule, and the GEMM
with an fp64 product of the DEQUANTISED operands (so only f32 accumulation order separates them).  The model-level
test reports what fp8 operands cost in depth accuracy; that figure is not held to the 1e-3 of the 16-bit path."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import matrix_eyes_amd as m
from mx_ref import dequant as _dequant, quantize_ref as _quantize_ref, read_scales as _read_scales, scale_bytes as _scale_bytes
from util import ctx_for, ptr, rel_l2

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


def _quantize_gpu(ctx, x16, weight_layout):
    rows, K = x16.shape
    d8 = torch.empty(rows, K, dtype=torch.uint8, device="cuda")
    n_scale = (rows if weight_layout else (rows + 127) // 128 * 128) * K // 32
    sc = torch.zeros(n_scale, dtype=torch.uint8, device="cuda")
    ctx._check(ctx.lib.me_op_quantize_fp8(ctx.handle, ptr(x16), rows, K, weight_layout, ptr(d8), ptr(sc)))
    ctx.synchronize()
    return d8, sc


@pytest.mark.parametrize("weight_layout", [0, 1])
def test_quantizer_is_the_mx_rule(weight_layout):
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(3 + weight_layout)
    rows, K = 192, 256
    x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 3)   # wide dynamic range
    x[5, 32:64] = 0.0                     # an all-zero block
    x[7, 0] = 60000.0                     # f16 extremes
    x[9, 64:96] = 6e-8
    x16 = x.half().cuda()
    d8, sc = _quantize_gpu(ctx, x16, weight_layout)
    q_ref, sb_ref = _quantize_ref(x16.cpu().float())
    sb = _read_scales(ctx, sc, rows, K, weight_layout)
    assert torch.equal(sb, sb_ref)
    got = d8.cpu().view(E4M3).float()
    want = q_ref.float()
    assert torch.equal(got, want)          # same e4m3 codes (compared as values: +0 == -0)
    # and the pair reproduces x to e4m3 precision: <= 2^-4 of the block maximum per element
    back = _dequant(d8.cpu().view(E4M3), sb)
    blockmax = x16.cpu().double().abs().reshape(rows, K // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(rows, K)
    assert float(((back - x16.cpu().double()).abs() / blockmax.clamp_min(1e-30)).max()) <= 2.0 ** -4


@pytest.mark.parametrize("shape", [(512, 768, 256), (1024, 1024, 1024), (1280, 256, 4096), (256, 3072, 1024)])
def test_linear_fp8_against_dequantised_operands(shape):
    """D = A8 . W8^T with block scales, all three epilogues, against the fp64 product of the dequantised operands"""
    M, N, K = shape
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(M + N + K)
    a16 = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).half().cuda()
    w16 = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
    bias = torch.randn(N, generator=g).cuda()
    gamma = (torch.rand(N, generator=g) * 0.2 + 0.05).cuda()
    a8, asc = _quantize_gpu(ctx, a16, 0)
    w8, wsc = _quantize_gpu(ctx, w16, 1)
    A = _dequant(a8.cpu().view(E4M3), _read_scales(ctx, asc, M, K, 0))
    W = _dequant(w8.cpu().view(E4M3), _read_scales(ctx, wsc, N, K, 1))
    ref = A @ W.T + bias.cpu().double()
    # (a) f16 output
    out16 = torch.empty(M, N, dtype=torch.float16, device="cuda")
    ctx._check(ctx.lib.me_op_linear_fp8(ctx.handle, M, N, K, ptr(a8), ptr(asc), ptr(w8), ptr(wsc), ptr(bias), ptr(out16),
                                        None, None, None, None))
    ctx.synchronize()
    err = (out16.cpu().double() - ref).abs()
    assert float((err / (ref.abs() * 2.0 ** -11 + 1e-3 * ref.abs().mean())).max()) < 1.6     # one f16 rounding + f32 sums
    # (b) residual update in f32
    x0 = torch.randn(M, N, generator=g)
    x32 = x0.clone().cuda()
    ctx._check(ctx.lib.me_op_linear_fp8(ctx.handle, M, N, K, ptr(a8), ptr(asc), ptr(w8), ptr(wsc), ptr(bias), None, None,
                                        None, ptr(gamma), ptr(x32)))
    ctx.synchronize()
    want = x0.double() + gamma.cpu().double() * ref
    assert float((x32.cpu().double() - want).abs().max() / want.abs().max()) < 3e-5    # f32 sums over K
    # (c) GELU then MX fp8 output, as the next GEMM's activation operand
    o8 = torch.empty(M, N, dtype=torch.uint8, device="cuda")
    osc = torch.zeros((M + 127) // 128 * 128 * N // 32, dtype=torch.uint8, device="cuda")
    ctx._check(ctx.lib.me_op_linear_fp8(ctx.handle, M, N, K, ptr(a8), ptr(asc), ptr(w8), ptr(wsc), ptr(bias), None, ptr(o8),
                                        ptr(osc), None, None))
    ctx.synchronize()
    act = F.gelu(ref)
    q_ref, sb_ref = _quantize_ref(act.float())
    sb = _read_scales(ctx, osc, M, N, 0)
    # the scale follows the block maximum, which is an f32 sum on the GPU and an f64 one here: a maximum that sits
    # on a power-of-two (or 1.75 x) boundary may land on the other side -- rare, and then by exactly one
    diff = (sb.int() - sb_ref.int()).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    got = _dequant(o8.cpu().view(E4M3), sb)
    blockmax = act.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
    assert float(((got - act).abs() / blockmax.clamp_min(1e-30)).max()) <= 2.0 ** -4 * 1.01 + 1e-6


def _scale_table(packed, rows, K, weight_layout):
    """_read_scales without the per-element ctypes call: the index formulas of csrc/mx_fp8.h (a_scale_index /
    w_scale_index) in numpy, spot-checked against me_op_scale_index"""
    host = packed.cpu().numpy()
    r = np.arange(rows, dtype=np.int64)[:, None]
    kb = np.arange(K // 32, dtype=np.int64)[None, :]
    if weight_layout:
        nt = rows // 64
        idx = (((kb >> 2) * nt + (r >> 6)) * 64 + (kb & 3) * 16 + (r & 15)) * 4 + ((r & 63) >> 4)
    else:
        mt = (rows + 127) // 128
        idx = (((kb >> 2) * mt + (r >> 7)) * 64 + (kb & 3) * 16 + (r & 15)) * 8 + ((r & 127) >> 4)
    return torch.from_numpy(host[idx])


@pytest.mark.parametrize("N,K,form", [(3072, 1024, "f16"), (4096, 1024, "gelu8"), (1024, 4096, "resid"), (1024, 1024, "resid")])
def test_linear_fp8_at_the_step_shapes_with_cold_caches(N, K, form):
    """The fp8 GEMM exactly as the encoder's merged ViT launches run it at one image: M = 21760 rows in three row
    segments (768 | 768 | 20224) with their own weights, scales, bias and gamma; (N, K) = qkv, fc1, fc2, proj.  Two
    different problems alternate and the L2 / Infinity Cache are flushed between launches: round 2's scale-load race
    (ME_RETIRE_SCALES) corrupted 15 - 40 % of the outputs exactly when the loads were slow -- first launch,
    cold caches -- and was right on every warm repeat, so a warm single-problem test cannot see it.  Every output
    element of every launch is compared with the f64 product of the dequantised operands (computed on the GPU in f64
    from the bytes the kernels read)."""
    import ctypes
    M, seg1, seg2 = 21760, 768, 1536
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(N + K)
    wsets = []
    for sgm in range(3):
        w16 = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
        w8, wsc = _quantize_gpu(ctx, w16, 1)
        tab = _scale_table(wsc, N, K, 1)
        if sgm == 0:      # the numpy layout formula is me_op_scale_index
            host = wsc.cpu().numpy()
            for r, kb in ((0, 0), (17, 3), (63, 5), (64, 4), (N - 1, K // 32 - 1), (N // 2 + 5, 9)):
                assert int(tab[r, kb]) == int(host[ctx.lib.me_op_scale_index(r, kb, N, 1)])
        W = _dequant(w8.cpu().view(E4M3), tab).cuda()
        wsets.append((w8, wsc, W, torch.randn(N, generator=g).cuda(), (torch.rand(N, generator=g) * 0.15 + 0.05).cuda()))
    probs = []
    for scale in (1.0, 3.0):
        a16 = (torch.randn(M, K, generator=g) * scale * torch.exp(torch.randn(M, 1, generator=g) * 0.5)).half().cuda()
        a8, asc = _quantize_gpu(ctx, a16, 0)
        atab = _scale_table(asc, M, K, 0)
        host = asc.cpu().numpy()
        for r, kb in ((0, 0), (129, 3), (M - 1, K // 32 - 1), (777, 6)):
            assert int(atab[r, kb]) == int(host[ctx.lib.me_op_scale_index(r, kb, M, 0)])
        A = _dequant(a8.cpu().view(E4M3), atab).cuda()
        ref = torch.empty(M, N, dtype=torch.float64, device="cuda")
        for lo, hi, ws in ((0, seg1, wsets[0]), (seg1, seg2, wsets[1]), (seg2, M, wsets[2])):
            ref[lo:hi] = A[lo:hi] @ ws[2].T + ws[3].double()
        probs.append((a8, asc, ref))
        del A, a16
    VP = ctypes.c_void_p * 3
    W8 = VP(*[w[0].data_ptr() for w in wsets]); WS = VP(*[w[1].data_ptr() for w in wsets])
    BI = VP(*[w[3].data_ptr() for w in wsets]); GA = VP(*[w[4].data_ptr() for w in wsets])
    gam = torch.cat([wsets[0][4].expand(seg1, N), wsets[1][4].expand(seg2 - seg1, N), wsets[2][4].expand(M - seg2, N)]).double()
    out16 = torch.empty(M, N, dtype=torch.float16, device="cuda")
    o8 = torch.empty(M, N, dtype=torch.uint8, device="cuda")
    osc = torch.zeros(M * N // 32, dtype=torch.uint8, device="cuda")
    x0 = torch.randn(M, N, generator=g).cuda()
    x32 = torch.empty_like(x0)
    for rep in range(6):
        a8, asc, ref = probs[rep % 2]
        if rep >= 2:
            torch.empty(512 << 20, dtype=torch.uint8, device="cuda").fill_(rep)       # flush L2 and the Infinity Cache
            torch.cuda.synchronize()
        if form == "f16":
            out16.fill_(float("nan"))
            torch.cuda.synchronize()
            ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, None,
                                                         ptr(out16), None, None, None))
            ctx.synchronize()
            err = (out16.double() - ref).abs()
            bad = err > (ref.abs() * 2.0 ** -10 + 2e-3 * ref.abs().mean())
        elif form == "resid":
            x32.copy_(x0)
            torch.cuda.synchronize()
            ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, GA,
                                                         None, None, None, ptr(x32)))
            ctx.synchronize()
            want = x0.double() + gam * ref
            bad = (x32.double() - want).abs() > 1e-4 * want.abs().max()
        else:
            o8.zero_(); osc.zero_()
            torch.cuda.synchronize()
            ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, None,
                                                         None, ptr(o8), ptr(osc), None))
            ctx.synchronize()
            act = F.gelu(ref)
            got = _dequant(o8.cpu().view(E4M3), _scale_table(osc, M, N, 0)).cuda()
            blockmax = act.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
            # half an e4m3 ulp of the block maximum, doubled where the block scale fell on the other side of a
            # power-of-two boundary (f32 sums here, f64 there: rare)
            bad = (got - act).abs() > blockmax * 2.0 ** -3 + 1e-6
        frac = float(bad.float().mean())
        print(form, (N, K), "launch", rep, "cold" if rep >= 2 else "warm-up", "bad fraction", frac)
        assert frac == 0.0, (form, N, K, rep, frac, bad.nonzero()[:4].tolist())


def test_layernorm_fp8():
    _layernorm_fp8_case(700, 1024)


@pytest.mark.parametrize("dim", [256, 512])
def test_layernorm_fp8_narrow_dims(dim):
    """the other two instantiations of layernorm_fp8_kernel (one and two passes of four elements per lane), same bounds; row
    counts that end inside a workgroup's four rows"""
    for rows in (700, 1, 3, 5, 1001):
        _layernorm_fp8_case(rows, dim)


def _layernorm_fp8_case(rows, dim):
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(rows, dim, generator=g) * 3 + 0.5)
    x[:, 17] += 40.0                      # an outlier channel, as DINOv2 has
    w, b = torch.randn(dim, generator=g) * 0.1 + 1, torch.randn(dim, generator=g) * 0.1
    y8 = torch.full((rows + 1, dim), 0xA5, dtype=torch.uint8, device="cuda")      # a guard row behind the output
    ys = torch.zeros((rows + 127) // 128 * 128 * dim // 32, dtype=torch.uint8, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()          # kept alive until the kernel has run
    ctx._check(ctx.lib.me_op_layernorm_fp8(ctx.handle, ptr(xd), ptr(wd), ptr(bd), ptr(y8), ptr(ys), rows, dim, 1e-5))
    ctx.synchronize()
    assert bool((y8[rows] == 0xA5).all())
    y8 = y8[:rows]
    ref = F.layer_norm(x.double(), (dim,), w.double(), b.double(), 1e-5)
    sb = _read_scales(ctx, ys, rows, dim, 0)
    diff = (sb.int() - _scale_bytes(ref.float().abs().reshape(rows, dim // 32, 32).amax(2)).int()).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    got = _dequant(y8.cpu().view(E4M3), sb)
    blockmax = ref.abs().reshape(rows, dim // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(rows, dim)
    assert float(((got - ref).abs() / blockmax).max()) <= 2.0 ** -4 * 1.01


def test_fp8_context_needs_wide_embeddings():
    with pytest.raises(m.MatrixEyesError) as e:
        m.Context(0, "fp8", m.ModelConfig.tiny())           # embed_dim 128 < one 256-wide tile
    assert e.value.code == 2


def test_extract_depth_fp8_small_model():
    """The whole path with fp8 ViT linears on a model the CPU oracle finishes in seconds (embed 256): finite,
    deterministic, close to the f16 path, and its depth error against the fp32 oracle REPORTED (fp8 operands carry 3
    significand bits: this is not the 1e-3 path)."""
    from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
    from oracle import depth_pro_oracle as O
    from util import depth_error_report, oracle_cfg
    cfg = m.ModelConfig(grid=8, embed_dim=256, num_heads=4, depth=4, tap_blocks=(1, 2), enc_dims=(64, 128, 128, 128),
                        dec_dim=256, head_dims=(32, 1))
    w = synthetic_checkpoint(cfg)
    rgb = synthetic_images(2, cfg.img_size)
    ref, ref_fov = O.extract_depth(O.preprocess_u8(rgb), None, w, oracle_cfg(cfg))
    res = {}
    for dtype in ("f16", "fp8"):
        ctx = m.Context(0, dtype, cfg)
        ctx.load_state_dict(w)
        d, fov = ctx.extract_depth(rgb, None, want_fov=True)
        d2, fov2 = ctx.extract_depth(rgb, None, want_fov=True)
        assert np.array_equal(d, d2) and np.array_equal(fov, fov2) and np.isfinite(d).all()
        one, _ = ctx.extract_depth(rgb[1:2], None, want_fov=True)
        assert np.array_equal(one[0], d[1])                   # batch == loop of batch one, fp8 too
        res[dtype] = (depth_error_report(d, ref.numpy()), fov)
        ctx.close()
    print("small model: f16", res["f16"][0], "fp8", res["fp8"][0], "fov", res["f16"][1], res["fp8"][1], ref_fov)
    assert res["f16"][0]["rel_l2"] < 2e-3
    assert res["f16"][0]["rel_l2"] < res["fp8"][0]["rel_l2"] < 0.1
    assert np.abs(res["fp8"][1] - ref_fov.numpy()).max() < 2.0


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 6, 9, 15])
def test_fp8_linears_mask_small_model(mask):
    """me_model_config.fp8_linears: any subset of {qkv, proj, fc1, fc2} on fp8, the rest on the 16-bit kernels with
    16-bit operands between them (an f16 fc1 feeding an fp8 fc2 is quantised by a separate pass, an fp8 fc1 feeding an
    f16 fc2 writes f16).  Every mask gives a finite depth closer to the f16 path than the all-fp8 path's bound, is
    deterministic, and a batch equals the loop of batch one."""
    from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
    cfg = m.ModelConfig(grid=8, embed_dim=256, num_heads=4, depth=4, tap_blocks=(1, 2), enc_dims=(64, 128, 128, 128),
                        dec_dim=256, head_dims=(32, 1), fp8_linears=mask)
    w = synthetic_checkpoint(cfg)
    rgb = synthetic_images(2, cfg.img_size)
    f16 = m.Context(0, "f16", cfg)
    f16.load_state_dict(w)
    ref = f16.extract_depth(rgb, None)
    f16.close()
    ctx = m.Context(0, "fp8", cfg)
    ctx.load_state_dict(w)
    d = ctx.extract_depth(rgb, None)
    assert np.isfinite(d).all() and np.array_equal(d, ctx.extract_depth(rgb, None))
    assert np.array_equal(ctx.extract_depth(rgb[1:2], None)[0], d[1])
    err = rel_l2(d, ref)
    print("fp8_linears", mask, "rel-L2 against the f16 path", err)
    assert 1e-4 < err < 0.1
    ctx.close()


def test_bcast_weights_rebuilds_the_fp8_arena():
    """on an fp8 context the e4m3 weight copies are DERIVED data -- me_bcast_weights (and
    me_weights_adopt) must re-quantise them from the 16-bit arena they have just received.  Here the receiving side of
    a broadcast is played on one GPU: a context loaded with checkpoint A gets checkpoint B's 16-bit arena written under
    it (its fp8 copies are now stale: the depth is neither A's nor B's), then me_bcast_weights runs with one rank --
    communicator, layout check, in-place broadcast, rebuild -- and the depth is bit for bit that of a context loaded
    with B directly."""
    from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
    cfg = m.ModelConfig(grid=8, embed_dim=256, num_heads=4, depth=4, tap_blocks=(1, 2), enc_dims=(64, 128, 128, 128),
                        dec_dim=256, head_dims=(32, 1))
    rgb = synthetic_images(1, cfg.img_size)
    b_ctx = m.Context(0, "fp8", cfg)
    b_ctx.load_state_dict(synthetic_checkpoint(cfg, seed=5))
    want = b_ctx.extract_depth(rgb, None)
    ctx = m.Context(0, "fp8", cfg)
    ctx.load_state_dict(synthetic_checkpoint(cfg, seed=6))
    a_depth = ctx.extract_depth(rgb, None)
    assert ctx.weight_arena_layout() == b_ctx.weight_arena_layout() != 0
    ctx.weight_arena_tensor().copy_(b_ctx.weight_arena_tensor())
    torch.cuda.synchronize()
    stale = ctx.extract_depth(rgb, None)             # 16-bit weights of B, fp8 linears still A's
    assert not np.array_equal(stale, want) and not np.array_equal(stale, a_depth)
    ctx.bcast_weights(ctx.rccl_unique_id(), 0, 1)
    assert np.array_equal(ctx.extract_depth(rgb, None), want)
    ctx.close()
    b_ctx.close()


@pytest.mark.parametrize("windows,tokens,heads", [(3, 577, 4), (5, 65, 2), (2, 130, 16), (1, 128, 2)])
def test_attention_fp8_output_equals_quantised_16bit_output(windows, tokens, heads):
    ctx = ctx_for("tiny", "f16")
    C, rows = heads * 64, windows * tokens
    g = torch.Generator().manual_seed(tokens + heads)
    qkv = (torch.randn(rows, 3 * C, generator=g) * 1.5).half().cuda()
    out16 = torch.empty(rows, C, dtype=torch.float16, device="cuda")
    nsc = (rows + 127) // 128 * 128 * C // 32
    want8 = torch.zeros(rows, C, dtype=torch.uint8, device="cuda"); want_s = torch.zeros(nsc, dtype=torch.uint8, device="cuda")
    got8 = torch.zeros_like(want8); got_s = torch.zeros_like(want_s)
    torch.cuda.synchronize()
    ctx._check(ctx.lib.me_op_attention(ctx.handle, ptr(qkv), ptr(out16), windows, tokens, heads))
    ctx._check(ctx.lib.me_op_quantize_fp8(ctx.handle, ptr(out16), rows, C, 0, ptr(want8), ptr(want_s)))
    ctx._check(ctx.lib.me_op_attention_fp8(ctx.handle, ptr(qkv), ptr(got8), ptr(got_s), windows, tokens, heads))
    ctx.synchronize()
    bad = (got8 != want8).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), int((got8 != want8).sum()))
    assert torch.equal(got_s, want_s)


_SEPARATE_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import matrix_eyes_amd as m
from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
cfg = m.ModelConfig(grid=8, embed_dim=256, num_heads=4, depth=4, tap_blocks=(1, 2), enc_dims=(64, 128, 128, 128),
                    dec_dim=256, head_dims=(32, 1))
cfg.fp8_linears = 15          # proj on fp8 too: the attention kernel then writes the projection's fp8 operand
ctx = m.Context(0, "fp8", cfg)
ctx.load_state_dict(synthetic_checkpoint(cfg))
d, fov = ctx.extract_depth(synthetic_images(2, cfg.img_size), None, want_fov=True)
np.save(sys.argv[2], d)
"""


def test_attention_writes_the_projection_operand_itself(tmp_path):
    """fp8 contexts: the attention kernel stores its output as MX fp8 bytes + block scales (values rounded to 16 bit
    first); ME_FP8_ATT_SEPARATE=1 runs the 16-bit store and the stand-alone quantiser instead.  Same depth, bit
    for bit, with and without the FOV head's third row segment."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for name, extra in (("fused", {}), ("separate", {"ME_FP8_ATT_SEPARATE": "1"})):
        path = str(tmp_path / (name + ".npy"))
        r = subprocess.run([sys.executable, "-c", _SEPARATE_CHILD, root, path], env=dict(os.environ, **extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("shape", [(352, 256, 128, 0, 0), (1000, 1024, 256, 0, 0), (1536, 512, 128, 512, 1024),
                                   (2300, 1024, 1024, 768, 0)])
def test_linear_residual_layernorm_fp8_fused(shape):
    """ME_DTYPE_FP8 contexts: the 16-bit projection's residual epilogue writes norm2 as fc1's MX fp8 operand
    (gemm_core.h resid_ln_epilogue, GemmParams::out8).  x32 is bit for bit the plain residual launch's; the bytes and
    scales are what me_op_layernorm_fp8 gives on those x32 rows, up to the last bit of a few elements (the two sum a
    row's statistics in a different order); dequantised they sit within half an e4m3 step of an fp64 LayerNorm; rows
    behind M are not written."""
    M, N, K, seg1, seg2 = shape
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(M + N + K + 1)
    a = torch.randn(M, K, generator=g).half().cuda()
    ws = [(torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda() for _ in range(3)]
    bs = [torch.randn(N, generator=g).cuda() for _ in range(3)]
    gs = [(0.05 + 0.15 * torch.rand(N, generator=g)).cuda() for _ in range(3)]
    lw = [(1.0 + 0.1 * torch.randn(N, generator=g)).cuda() for _ in range(3)]
    lb = [(0.1 * torch.randn(N, generator=g)).cuda() for _ in range(3)]
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    x0 = torch.randn(M, N, generator=g) * 2.0
    x0[:, 7] += 40.0
    x0[::3] *= 10.0
    x0 = x0.cuda()
    plain, fused = x0.clone(), x0.clone()
    mt = (M + 127) // 128
    xn8 = torch.full((M + 1, N), 0x55, dtype=torch.uint8, device="cuda")       # a guard row behind the output
    xs = torch.zeros(mt * 128 * N // 32, dtype=torch.uint8, device="cuda")
    eps = 1e-5
    torch.cuda.synchronize()
    ctx._check(ctx.lib.me_op_linear_segments(ctx.handle, M, N, K, ptr(a), seg1, seg2, arr(ws), arr(bs), arr(gs), None, ptr(plain), 0, 10))
    ctx._check(ctx.lib.me_op_linear_residual_layernorm_fp8(ctx.handle, M, N, K, ptr(a), seg1, seg2, arr(ws), arr(bs), arr(gs), arr(lw),
                                                           arr(lb), eps, ptr(fused), ptr(xn8), ptr(xs)))
    ctx.synchronize()
    assert ctx.status_flags() == 0
    assert torch.equal(fused, plain)
    assert bool((xn8[M] == 0x55).all())
    bounds = [0, seg1 if seg1 else M, (seg2 if seg2 else M) if seg1 else M, M]
    ref = torch.empty(M, N, dtype=torch.float64)
    xd = fused.double().cpu()
    for i in range(3):
        lo, hi = bounds[i], bounds[i + 1]
        if hi > lo:
            ref[lo:hi] = F.layer_norm(xd[lo:hi], (N,), lw[i].double().cpu(), lb[i].double().cpu(), eps)
    sb = _read_scales(ctx, xs, M, N, 0)
    diff = (sb.int() - _scale_bytes(ref.float().abs().reshape(M, N // 32, 32).amax(2)).int()).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    got = _dequant(xn8[:M].cpu().view(E4M3), sb)
    blockmax = ref.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
    assert float(((got - ref).abs() / blockmax).max()) <= 2.0 ** -4 * 1.01
    # the stand-alone LayerNorm -> fp8 kernel on the same rows (one weight set: no segments)
    if seg1 == 0:
        y8 = torch.empty(M, N, dtype=torch.uint8, device="cuda")
        ys = torch.zeros_like(xs)
        ctx._check(ctx.lib.me_op_layernorm_fp8(ctx.handle, ptr(fused), ptr(lw[0]), ptr(lb[0]), ptr(y8), ptr(ys), M, N, eps))
        ctx.synchronize()
        assert float((ys != xs).float().mean()) < 1e-3
        assert float((y8 != xn8[:M]).float().mean()) < 2e-3
    # again from the same input: the same bytes
    again = x0.clone()
    xn8b = torch.empty(M, N, dtype=torch.uint8, device="cuda")
    xsb = torch.zeros_like(xs)
    torch.cuda.synchronize()
    ctx._check(ctx.lib.me_op_linear_residual_layernorm_fp8(ctx.handle, M, N, K, ptr(a), seg1, seg2, arr(ws), arr(bs), arr(gs), arr(lw),
                                                           arr(lb), eps, ptr(again), ptr(xn8b), ptr(xsb)))
    ctx.synchronize()
    assert torch.equal(again, fused) and torch.equal(xn8b, xn8[:M]) and torch.equal(xsb, xs)
    assert ctx.status_flags() == 0


def _fp8_problem(ctx, g, M, N, K, nseg):
    """quantised operands of an fp8 linear over `nseg` row segments + the dequantised f64 matrices"""
    a16 = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 0.5)).half().cuda()
    a8, asc = _quantize_gpu(ctx, a16, 0)
    A = _dequant(a8.cpu().view(E4M3), _scale_table(asc, M, K, 0)).cuda()
    wsets = []
    for _ in range(nseg):
        w16 = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
        w8, wsc = _quantize_gpu(ctx, w16, 1)
        W = _dequant(w8.cpu().view(E4M3), _scale_table(wsc, N, K, 1)).cuda()
        wsets.append((w8, wsc, W, torch.randn(N, generator=g).cuda(), (torch.rand(N, generator=g) * 0.15 + 0.05).cuda()))
    while len(wsets) < 3:
        wsets.append(wsets[0])
    return a8, asc, A, wsets


@pytest.mark.parametrize("shape", [(21760, 1024, 4096, 768, 1536), (21760, 4096, 1024, 768, 1536), (21760, 3072, 1024, 768, 1536),
                                   (5120, 1024, 1024, 0, 0)])
def test_linear_fp8_tall_tile_is_bit_identical_to_the_256_row_tile(shape):
    """gemm_pp8t_kernel (352-row tile, csrc/gemm_fp8.hip) against gemm_pp8_kernel on the same operands, the
    three epilogues, at the step's shapes with its three row segments: the same K order per output element, so the same bits.
    ME_FP8_TALL = 0 / 1 picks the tile (read per launch)."""
    import os
    M, N, K, seg1, seg2 = shape
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(M + N + K + 3)
    a8, asc, A, wsets = _fp8_problem(ctx, g, M, N, K, 3 if seg2 else 1)
    VP = C.c_void_p * 3
    W8 = VP(*[w[0].data_ptr() for w in wsets]); WS = VP(*[w[1].data_ptr() for w in wsets])
    BI = VP(*[w[3].data_ptr() for w in wsets]); GA = VP(*[w[4].data_ptr() for w in wsets])
    x0 = torch.randn(M, N, generator=g).cuda()
    got = {}
    old = os.environ.get("ME_FP8_TALL")
    try:
        for tall in ("0", "1"):
            os.environ["ME_FP8_TALL"] = tall
            out16 = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda")
            o8 = torch.zeros(M, N, dtype=torch.uint8, device="cuda")
            osc = torch.zeros(M * N // 32, dtype=torch.uint8, device="cuda")
            x32 = x0.clone()
            torch.cuda.synchronize()
            ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, None,
                                                         ptr(out16), None, None, None))
            ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, None,
                                                         None, ptr(o8), ptr(osc), None))
            ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, GA,
                                                         None, None, None, ptr(x32)))
            ctx.synchronize()
            got[tall] = (out16, o8, osc, x32)
    finally:
        if old is None:
            os.environ.pop("ME_FP8_TALL", None)
        else:
            os.environ["ME_FP8_TALL"] = old
    assert bool(torch.isfinite(got["1"][0]).all())
    for a, b in zip(got["0"], got["1"]):
        assert torch.equal(a, b)
    # and against the f64 product of the dequantised operands (the first segment's rows)
    hi = seg1 if seg1 else M
    ref = A[:hi] @ wsets[0][2].T + wsets[0][3].double()
    err = (got["1"][0][:hi].double() - ref).abs()
    assert float((err / (ref.abs() * 2.0 ** -10 + 2e-3 * ref.abs().mean())).max()) < 1.0


@pytest.mark.parametrize("shape", [(1000, 1024, 256, 0, 0), (1536, 512, 512, 512, 1024), (2300, 1024, 1024, 768, 0),
                                   (21760, 1024, 4096, 768, 1536)])
def test_linear_fp8_residual_layernorm_fused(shape):
    """The fp8 fc2 with the next block's norm1 in its residual epilogue (gemm_pp8t_kernel<..., LNF>): x32 is bit for bit the plain
    fp8 residual launch's (ragged M included: the tall tile clamps its rows); the bytes and scales are what me_op_layernorm_fp8
    gives on those x32 rows up to the last bit of a few elements; dequantised they sit within half an e4m3 step of an fp64
    LayerNorm; rows behind M are not written; a second launch from the same input gives the same bytes."""
    import os
    M, N, K, seg1, seg2 = shape
    ctx = ctx_for("tiny", "f16")
    g = torch.Generator().manual_seed(M + N + K + 7)
    nseg = 3 if seg2 else (2 if seg1 else 1)
    a8, asc, A, wsets = _fp8_problem(ctx, g, M, N, K, nseg)
    lw = [(1.0 + 0.1 * torch.randn(N, generator=g)).cuda() for _ in range(3)]
    lb = [(0.1 * torch.randn(N, generator=g)).cuda() for _ in range(3)]
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    W8 = arr([w[0] for w in wsets]); WS = arr([w[1] for w in wsets]); BI = arr([w[3] for w in wsets]); GA = arr([w[4] for w in wsets])
    x0 = torch.randn(M, N, generator=g) * 2.0
    x0[:, 7] += 40.0
    x0[::3] *= 10.0
    x0 = x0.cuda()
    plain, fused = x0.clone(), x0.clone()
    mt = (M + 127) // 128
    xn8 = torch.full((M + 1, N), 0x55, dtype=torch.uint8, device="cuda")       # a guard row behind the output
    xs = torch.zeros(mt * 128 * N // 32, dtype=torch.uint8, device="cuda")
    eps = 1e-5
    old = os.environ.get("ME_FP8_TALL")
    os.environ["ME_FP8_TALL"] = "1"
    try:
        torch.cuda.synchronize()
        ctx._check(ctx.lib.me_op_linear_fp8_segments(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, GA, None, None,
                                                     None, ptr(plain)))
    finally:
        if old is None:
            os.environ.pop("ME_FP8_TALL", None)
        else:
            os.environ["ME_FP8_TALL"] = old
    ctx._check(ctx.lib.me_op_linear_fp8_residual_layernorm(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, GA,
                                                           arr(lw), arr(lb), eps, ptr(fused), ptr(xn8), ptr(xs)))
    ctx.synchronize()
    assert ctx.status_flags() == 0
    assert torch.equal(fused, plain)
    assert bool((xn8[M] == 0x55).all())
    bounds = [0, seg1 if seg1 else M, (seg2 if seg2 else M) if seg1 else M, M]
    # the residual update itself against f64
    want = x0.double()
    for i in range(3):
        lo, hi = bounds[i], bounds[i + 1]
        if hi > lo:
            want[lo:hi] += wsets[i][4].double() * (A[lo:hi] @ wsets[i][2].T + wsets[i][3].double())
    assert float((fused.double() - want).abs().max() / want.abs().max()) < 3e-5
    ref = torch.empty(M, N, dtype=torch.float64)
    xd = fused.double().cpu()
    for i in range(3):
        lo, hi = bounds[i], bounds[i + 1]
        if hi > lo:
            ref[lo:hi] = F.layer_norm(xd[lo:hi], (N,), lw[i].double().cpu(), lb[i].double().cpu(), eps)
    sb = _scale_table(xs, M, N, 0)
    diff = (sb.int() - _scale_bytes(ref.float().abs().reshape(M, N // 32, 32).amax(2)).int()).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    got = _dequant(xn8[:M].cpu().view(E4M3), sb)
    blockmax = ref.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
    assert float(((got - ref).abs() / blockmax).max()) <= 2.0 ** -4 * 1.01
    if seg1 == 0:   # the stand-alone LayerNorm -> fp8 kernel on the same rows (one weight set: no segments)
        y8 = torch.empty(M, N, dtype=torch.uint8, device="cuda")
        ys = torch.zeros_like(xs)
        ctx._check(ctx.lib.me_op_layernorm_fp8(ctx.handle, ptr(fused), ptr(lw[0]), ptr(lb[0]), ptr(y8), ptr(ys), M, N, eps))
        ctx.synchronize()
        assert float((ys != xs).float().mean()) < 1e-3
        assert float((y8 != xn8[:M]).float().mean()) < 2e-3
    again = x0.clone()
    xn8b = torch.empty(M, N, dtype=torch.uint8, device="cuda")
    xsb = torch.zeros_like(xs)
    torch.cuda.synchronize()
    ctx._check(ctx.lib.me_op_linear_fp8_residual_layernorm(ctx.handle, M, N, K, ptr(a8), ptr(asc), seg1, seg2, W8, WS, BI, GA,
                                                           arr(lw), arr(lb), eps, ptr(again), ptr(xn8b), ptr(xsb)))
    ctx.synchronize()
    assert torch.equal(again, fused) and torch.equal(xn8b, xn8[:M]) and torch.equal(xsb, xs)
    assert ctx.status_flags() == 0
