"""Red-zone tests (-m gpu): every kernel-level entry of include/matrix_eyes_hip_ops.h that takes a device pointer, with EVERY
pointer it takes -- operands, bias, gamma, LayerNorm weights, scale tables, f_norm, the members of pointer arrays -- the
payload of a tests/redzone.py Fence: 1 MiB of a known byte in front of and behind it.  Each call runs twice on the same input
values, once between 0xFF fences (NaN in every type the library reads) and once between 0x00 fences, and must

  (a) return ME_OK and meet the tolerance its existing test holds it to (cited at each case; none is invented here),
  (b) give bit-identical output payloads under both fills,
  (c) leave every guard byte of every fence, inputs included, as it was,
  (d) leave every input payload as it was (x32 of the residual forms is the documented in-place operand),
  (e) leave the elements the header documents as not written at the fill, write every other one, and under 0xFF leave no NaN.

The other kernel tests allocate operands at their exact size from torch's pool: a read past an operand lands in a live
neighbour full of finite numbers and `0 * neighbour` vanishes.  Here it is NaN under one fill and 0 under the other.

Shapes are the smallest at which an index can leave an operand: one row, ragged last tiles, one row past the 352-row tile, N off
the 8-element store, maps smaller than a tile, one token, one token past a key tile.  Tile ids come from tile_choice_cases.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layout_refs as R
import redzone as RZ
import row_segments_ref as RS
import test_gpu_convt_pair as CP
import test_gpu_fp8 as F8
import test_gpu_layout as LT
import test_gpu_split_forms as SF
import tile_choice_cases as TC
import weight_pack_cases as W
from mx_ref import E4M3, dequant, quantize_ref, scale_bytes
from test_gpu_ops import OUT_EPS, QSCALE
from util import TORCH16, ctx_for, max_abs_rel, max_err_over_max, pack_conv, pack_convt, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
F32, U8 = torch.float32, torch.uint8

# every me_op_* entry with a device pointer among its arguments and the test here that fences it; test_every_entry_is_fenced
# holds the list to matrix_eyes_amd/_lib.py
COVERED = {
    "me_op_linear": "test_linear", "me_op_linear_residual": "test_linear_residual",
    "me_op_linear_scaled_cols": "test_linear_scaled_cols", "me_op_linear_split": "test_linear_split",
    "me_op_linear_segments": "test_linear_segments", "me_op_linear_residual_layernorm": "test_linear_residual_layernorm",
    "me_op_linear_residual_layernorm_fp8": "test_linear_residual_layernorm", "me_op_patch_embed": "test_patch_embed",
    "me_op_conv2d": "test_conv2d", "me_op_conv2d_forms": "test_conv2d", "me_op_conv_transpose2x2": "test_conv_transpose",
    "me_op_conv_transpose2x2_forms": "test_conv_transpose_forms", "me_op_conv_transpose2x2_forms_wrap": "test_conv_transpose_forms",
    "me_op_conv_transpose2x2_pair": "test_conv_transpose_pair", "me_op_head_final": "test_head_final",
    "me_op_attention": "test_attention", "me_op_attention_prescaled": "test_attention", "me_op_attention_fp8": "test_attention_fp8",
    "me_op_attention_segments": "test_attention_segments", "me_op_layernorm": "test_layernorm",
    "me_op_layernorm_fp8": "test_layernorm_fp8", "me_op_layernorm_segments": "test_layernorm_segments",
    "me_op_quantize_fp8": "test_quantize_fp8", "me_op_linear_fp8": "test_linear_fp8",
    "me_op_linear_fp8_segments": "test_linear_fp8_segments", "me_op_linear_fp8_residual_layernorm": "test_linear_fp8_residual_layernorm",
    "me_op_bilinear": "test_bilinear", "me_op_patchify": "test_patchify", "me_op_patchify_windows": "test_patchify",
    "me_op_cls_rows": "test_cls_rows", "me_op_merge": "test_merge", "me_op_nchw32_to_nhwc": "test_layout_changes",
    "me_op_nhwc16_to_nchw32": "test_layout_changes", "me_op_nhwc32_to_nchw32": "test_layout_changes",
    "me_op_nhwc32_to_16b": "test_layout_changes", "me_op_concat_channels": "test_concat_and_fov_add",
    "me_op_fov_add": "test_concat_and_fov_add", "me_op_fov_final": "test_fov_final", "me_op_cast_to16": "test_casts",
    "me_op_cast_to32": "test_casts", "me_op_exclusive_scan_u32": "test_exclusive_scan", "me_op_ply_pack": "test_ply_pack",
    "me_op_format_f64": "test_format_f64", "me_op_weight_pack": "test_weight_pack", "me_op_png_unfilter": "test_png_unfilter",
    "me_op_jpeg_entropy": "test_jpeg_entropy",
}
# no device pointer: host arrays only, or no pointer at all
HOST_ONLY = {"me_op_scale_index", "me_op_lanczos3_table", "me_op_jpeg_decode_host", "me_op_jpeg_coefficients_host",
             "me_op_png_decode_host", "me_op_jpeg_encode_host", "me_op_weight_pack_host", "me_op_legacy_noise_host",
             "me_op_gemm_config_count", "me_op_gemm_config_name"}


def test_every_entry_is_fenced():
    """A new me_op_* entry in _lib.py must be listed here: with a fence case, or among the host-only ones."""
    import matrix_eyes_amd._lib as L
    names = set()
    for v in vars(L).values():
        if isinstance(v, dict):
            names |= {k for k in v if isinstance(k, str) and k.startswith("me_op_")}
    assert "me_op_linear" in names and "me_op_weight_pack" in names
    assert not (set(COVERED) & HOST_ONLY)
    assert names == set(COVERED) | HOST_ONLY, (sorted(names - set(COVERED) - HOST_ONLY), sorted((set(COVERED) | HOST_ONLY) - names))
    for name, test in COVERED.items():
        assert callable(globals().get(test)), (name, test)


@pytest.fixture(autouse=True)
def _clear_status():
    """a case that fails on a NaN read may leave the contexts' overflow bit up: the next test starts clean"""
    _TILE.clear()
    yield
    for d in DTYPES:
        ctx_for("tiny", d).status_flags()


# ---------------------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------------------
def p(t, offset_bytes=0):
    return C.c_void_p(t.data_ptr() + offset_bytes) if t is not None else C.c_void_p(0)


def arr3(ts):
    return (C.c_void_p * 3)(*[t.data_ptr() if t is not None else None for t in ts])


_TILE = []
CALLED = set()      # the me_op_* entries called inside run_both so far


class _Recorder:
    """the library, noting the name of every entry a fenced call asks it for"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        CALLED.add(name)
        return getattr(self._lib, name)



def tile(nbytes):
    """Every case states the bytes of an operand that one tile of its kernel spans -- what an over-read that is still in spec
    (a clamped row, a halo, a padded scale tile) could reach behind the operand: redzone.footprint holds it below half a guard.
    run_both refuses a case that has not stated it."""
    _TILE.append(RZ.footprint(int(nbytes)))


def run_both(ctx, build):
    """build(fs) -> (call, {name: output view}) on the FenceSet fs; runs it under both fills and checks (a)'s return code, (c)
    and (d).  Returns {fill: outputs}."""
    assert _TILE, "the case has not stated its tile footprint (tile())"
    res = {}
    real = ctx.lib
    for fill in RZ.FILLS:
        fs = RZ.FenceSet(fill)
        call, outs = build(fs)
        torch.cuda.synchronize()            # the fences were filled on torch's stream, the entry runs on the context's
        ctx.lib = _Recorder(real)           # which entries the case really calls: test_every_entry_was_called_between_fences
        try:
            rc = call()
        finally:
            ctx.lib = real
        ctx.synchronize()
        assert rc == 0, (rc, ctx.lib.me_last_error(ctx.handle))
        fs.check()
        res[fill] = outs
    return res


def settle(res, masks=None, raw=()):
    """(b) and (e) over the outputs of run_both.  masks[name]: True where the entry writes (default: everywhere), of the output's
    shape or of its leading dimensions; raw: outputs of bytes or integers, in which a written element may equal the fill.
    Returns the outputs of the 0xFF run."""
    masks = masks or {}
    ff, zz = res[0xFF], res[0x00]
    for name, a in ff.items():
        b = zz[name]
        m = masks.get(name)
        if m is None:
            m = torch.ones(a.shape, dtype=torch.bool, device=a.device)
        else:
            m = m.to(a.device)
            while m.dim() < a.dim():
                m = m.unsqueeze(-1)
            m = m.expand(a.shape)
        fa, fb = RZ.is_fill(a, 0xFF), RZ.is_fill(b, 0x00)
        assert bool(fa[~m].all()) and bool(fb[~m].all()), f"{name}: an element documented as not written was written"
        if name not in raw:
            assert not bool(fa[m].any()), f"{name}: {int(fa[m].sum())} elements were not written"
            if a.is_floating_point():
                assert not bool(torch.isnan(a.float()[m]).any()), f"{name}: NaN in the output under the 0xFF fill"
        size = a.element_size()
        same = (a.contiguous().view(U8).reshape(-1, size) == b.contiguous().view(U8).reshape(-1, size)).all(dim=1).reshape(a.shape)
        bad = m & ~same
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements depend on the fill, first at {bad.nonzero()[0].tolist()}"
    return ff


def tile_ids(amode, epi):
    return [-1] + [i for i in sorted(TC.ADMITS) if (amode, epi) in TC.ADMITS[i] and i not in TC.HALO_IDS]


LINEAR_IDS = tile_ids(TC.A_PLAIN, TC.EPI_STORE)
RESID_IDS = tile_ids(TC.A_PLAIN, TC.EPI_RESID_SCALE)
CONV_IDS = tile_ids(TC.A_CONV, TC.EPI_STORE)
CONVT_IDS = tile_ids(TC.A_PLAIN, TC.EPI_CONVT)
EMBED_IDS = tile_ids(TC.A_PLAIN, TC.EPI_PATCH_EMBED)


def gemm_operands(dtype, M, N, K, seed, sets=1):
    """host tensors: a [M][K] and `sets` of (w [N][K], bias, gamma) in the 16-bit type / f32, and x [M][N]"""
    T = TORCH16[dtype]
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(T)
    ws = [(torch.randn(N, K, generator=g) / math.sqrt(K)).to(T) for _ in range(sets)]
    bs = [torch.randn(N, generator=g) for _ in range(sets)]
    gs = [0.05 + 0.15 * torch.rand(N, generator=g) for _ in range(sets)]
    x = torch.randn(M, N, generator=g)
    tile(352 * K * 2)                       # one row tile of the tallest configuration
    return a, ws, bs, gs, x


def seg_bounds(M, seg1, seg2):
    return [0, seg1 if seg1 else M, (seg2 if seg2 else M) if seg1 else M, M]


def seg_linear_ref(a, ws, bs, M, seg1, seg2):
    """fp64 A W^T + bias per row segment (test_gpu_ops.py _segmented_linear)"""
    ref = torch.empty(M, ws[0].shape[0], dtype=torch.float64)
    b = seg_bounds(M, seg1, seg2)
    for i in range(3):
        if b[i + 1] > b[i]:
            ref[b[i]:b[i + 1]] = a[b[i]:b[i + 1]].double() @ ws[i].double().T + bs[i].double()
    return ref


def per_row(vs, M, seg1, seg2):
    """[M][N]: row m holds the vector of its segment"""
    b = seg_bounds(M, seg1, seg2)
    return torch.cat([vs[i].double().expand(b[i + 1] - b[i], -1) for i in range(3) if b[i + 1] > b[i]])


def act_scale_mask(rows, K):
    """the written positions of an activation-layout scale table of `rows` rows (csrc/mx_fp8.h a_scale_index, as
    test_gpu_fp8.py _scale_table states it): ceil(rows / 128) * 128 * K / 32 bytes, those of the rows behind `rows` not written"""
    mt = (rows + 127) // 128
    r = np.arange(rows, dtype=np.int64)[:, None]
    kb = np.arange(K // 32, dtype=np.int64)[None, :]
    idx = (((kb >> 2) * mt + (r >> 7)) * 64 + (kb & 3) * 16 + (r & 15)) * 8 + ((r & 127) >> 4)
    m = torch.zeros(mt * 128 * K // 32, dtype=torch.bool)
    m[torch.from_numpy(idx.ravel())] = True
    return m, idx


# ---------------------------------------------------------------------------------------------------------------------
# GEMM family
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", LINEAR_IDS)
@pytest.mark.parametrize("shape", [(1, 4, 64, 0), (65, 132, 192, 1), (353, 260, 128, 0)])
def test_linear(dtype, cfg, shape):
    """out16 and out32 together; GELU on the middle case.  Bounds: test_gpu_ops.py test_linear (2e-5 / 16 roundings of rms),
    test_linear_gelu (2e-5 absolute on the f32 copy), test_tall_tile_352 (the 16-bit copy under GELU)."""
    M, N, K, act = shape
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, ws, bs, _, _ = gemm_operands(dtype, M, N, K, M + N + K)

    def build(fs):
        A, Wt, b = fs.inp(a), fs.inp(ws[0]), fs.inp(bs[0])
        o16, o32 = fs.out(T, (M, N)), fs.out(F32, (M, N))
        return (lambda: ctx.lib.me_op_linear(ctx.handle, M, N, K, p(A), p(Wt), p(b), p(o16), p(o32), act, cfg)), {"out16": o16, "out32": o32}

    got = settle(run_both(ctx, build))
    ref = a.double() @ ws[0].double().T + bs[0].double()
    if act:
        ref = F.gelu(ref)
        assert float((got["out32"].cpu().double() - ref).abs().max()) < 2e-5
    else:
        assert max_abs_rel(got["out32"].cpu(), ref) < 2e-5
    assert max_abs_rel(got["out16"].float().cpu(), ref) < 4 * OUT_EPS[dtype] * 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", RESID_IDS)
@pytest.mark.parametrize("shape", [(65, 132, 192), (353, 256, 128)])
def test_linear_residual(dtype, cfg, shape):
    """x32 += gamma * (A W^T + bias) in place; bound: test_gpu_ops.py test_linear_residual (2e-5 of rms)"""
    M, N, K = shape
    ctx = ctx_for("tiny", dtype)
    a, ws, bs, gs, x = gemm_operands(dtype, M, N, K, M + N + K + 1)

    def build(fs):
        A, Wt, b, g_ = fs.inp(a), fs.inp(ws[0]), fs.inp(bs[0]), fs.inp(gs[0])
        X = fs.inout(x)
        return (lambda: ctx.lib.me_op_linear_residual(ctx.handle, M, N, K, p(A), p(Wt), p(b), p(g_), p(X), cfg)), {"x32": X}

    got = settle(run_both(ctx, build))
    ref = x.double() + gs[0].double() * (a.double() @ ws[0].double().T + bs[0].double())
    assert max_abs_rel(got["x32"].cpu(), ref) < 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", LINEAR_IDS)
def test_linear_scaled_cols(dtype, cfg):
    """(65, 384, 128) with the first 128 columns scaled; bounds: test_gpu_ops.py test_linear_scaled_cols"""
    M, N, K, qcols = 65, 384, 128, 128
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, ws, bs, _, _ = gemm_operands(dtype, M, N, K, 17)

    def build(fs):
        A, Wt, b = fs.inp(a), fs.inp(ws[0]), fs.inp(bs[0])
        o = fs.out(T, (M, N))
        return (lambda: ctx.lib.me_op_linear_scaled_cols(ctx.handle, M, N, K, p(A), p(Wt), p(b), p(o), qcols, QSCALE, cfg)), {"out16": o}

    got = settle(run_both(ctx, build))["out16"].float().cpu()
    ref = a.double() @ ws[0].double().T + bs[0].double()
    ref[:, :qcols] *= QSCALE
    assert max_err_over_max(got, ref) < 1.5 * OUT_EPS[dtype]
    assert rel_l2(got[:, :qcols], ref[:, :qcols]) < OUT_EPS[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", LINEAR_IDS)
def test_linear_split(dtype, cfg):
    """(65, 132, 128): [hi | lo] rows of 2 N and the f32 copy; bounds: test_gpu_split_forms.py linear_split_case"""
    M, N, K = 65, 132, 128
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, ws, bs, _, _ = gemm_operands(dtype, M, N, K, 23)

    def build(fs):
        A, Wt, b = fs.inp(a), fs.inp(ws[0]), fs.inp(bs[0])
        o16, o32 = fs.out(T, (M, 2 * N)), fs.out(F32, (M, N))
        return (lambda: ctx.lib.me_op_linear_split(ctx.handle, M, N, K, p(A), p(Wt), p(b), p(o16), p(o32), 0, cfg)), {"out16": o16, "out32": o32}

    got = settle(run_both(ctx, build))
    ref = a.double() @ ws[0].double().T + bs[0].double()
    assert max_abs_rel(got["out32"].cpu(), ref) < SF.LIN_BOUND
    SF.check_16bit(got["out16"], ref, T, 2, SF.LIN_BOUND, False, got["out32"], f"linear_split {dtype} cfg {cfg}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("resid", [0, 1])
@pytest.mark.parametrize("M,seg1,seg2,cfg", [(200, 64, 192, TC.CFG_64), (200, 64, 192, TC.CFG_RING64), (705, 100, 353, TC.CFG_PP352)])
def test_linear_segments(dtype, resid, M, seg1, seg2, cfg):
    """Three row segments with their own weights, boundaries on the 64-row tiles' grid and, for the 352-row tile, anywhere; both
    forms.  Bounds: test_gpu_ops.py test_tall_tile_352."""
    N, K = 132, 128
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, ws, bs, gs, x = gemm_operands(dtype, M, N, K, M + cfg, sets=3)

    def build(fs):
        A = fs.inp(a)
        Ws, Bs, Gs = [fs.inp(w) for w in ws], [fs.inp(b) for b in bs], [fs.inp(g_) for g_ in gs]
        if resid:
            X = fs.inout(x)
            return (lambda: ctx.lib.me_op_linear_segments(ctx.handle, M, N, K, p(A), seg1, seg2, arr3(Ws), arr3(Bs), arr3(Gs), None, p(X), 0,
                                                          cfg)), {"x32": X}
        o = fs.out(T, (M, N))
        return (lambda: ctx.lib.me_op_linear_segments(ctx.handle, M, N, K, p(A), seg1, seg2, arr3(Ws), arr3(Bs), arr3(Gs), p(o), None, 1,
                                                      cfg)), {"out16": o}

    got = settle(run_both(ctx, build))
    y = seg_linear_ref(a, ws, bs, M, seg1, seg2)
    if resid:
        assert max_abs_rel(got["x32"].cpu(), x.double() + per_row(gs, M, seg1, seg2) * y) < 2e-5
    else:
        assert max_abs_rel(got["out16"].float().cpu(), F.gelu(y)) < 4 * OUT_EPS[dtype] * 4


# the fp8 output forms of the 16-bit kernels are what an ME_DTYPE_FP8 context runs, whose 16-bit type is f16: their own tests
# (test_gpu_fp8.py, test_gpu_row_segments.py) run them on an f16 context, and so do these
DTYPE_FORMS = [("f16", 0), ("bf16", 0), ("f16", 1)]


@pytest.mark.parametrize("dtype,fp8", DTYPE_FORMS)
@pytest.mark.parametrize("M,N,K,seg1,seg2", [(353, 256, 128, 0, 0), (705, 512, 128, 100, 353)])
def test_linear_residual_layernorm(dtype, fp8, M, N, K, seg1, seg2):
    """The residual update with the next LayerNorm in the launch, 16-bit and MX fp8 rows.  Bounds: x32 as test_tall_tile_352
    (2e-5 of rms); the normalised rows as test_gpu_ops.py test_linear_residual_layernorm_fused, against an fp64 LayerNorm of
    the x32 the launch wrote; the fp8 rows as test_gpu_fp8.py test_linear_residual_layernorm_fp8_fused."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, ws, bs, gs, _ = gemm_operands(dtype, M, N, K, M + N + K + 5, sets=3)
    g = torch.Generator().manual_seed(M + 3)
    lw = [1.0 + 0.1 * torch.randn(N, generator=g) for _ in range(3)]
    lb = [0.1 * torch.randn(N, generator=g) for _ in range(3)]
    x0 = torch.randn(M, N, generator=g) * 2.0
    x0[:, 7] += 40.0
    x0[::3] *= 10.0
    eps = 1e-5
    smask, sidx = act_scale_mask(M, N)

    def build(fs):
        A = fs.inp(a)
        Ws, Bs, Gs = [fs.inp(w) for w in ws], [fs.inp(b) for b in bs], [fs.inp(g_) for g_ in gs]
        Lw, Lb = [fs.inp(w) for w in lw], [fs.inp(b) for b in lb]
        X = fs.inout(x0)
        if fp8:
            o8, os_ = fs.out(U8, (M, N)), fs.out(U8, (smask.numel(),))
            return (lambda: ctx.lib.me_op_linear_residual_layernorm_fp8(ctx.handle, M, N, K, p(A), seg1, seg2, arr3(Ws), arr3(Bs), arr3(Gs),
                                                                        arr3(Lw), arr3(Lb), eps, p(X), p(o8), p(os_))), \
                {"x32": X, "xn8": o8, "xn_scale": os_}
        o = fs.out(T, (M, N))
        return (lambda: ctx.lib.me_op_linear_residual_layernorm(ctx.handle, M, N, K, p(A), seg1, seg2, arr3(Ws), arr3(Bs), arr3(Gs),
                                                                arr3(Lw), arr3(Lb), eps, p(X), p(o))), {"x32": X, "xn16": o}

    ctx.status_flags()
    got = settle(run_both(ctx, build), masks={"xn_scale": smask})
    assert ctx.status_flags() == 0
    x32 = got["x32"].cpu()
    assert max_abs_rel(x32, x0.double() + per_row(gs, M, seg1, seg2) * seg_linear_ref(a, ws, bs, M, seg1, seg2)) < 2e-5
    b = seg_bounds(M, seg1, seg2)
    ref = torch.empty(M, N, dtype=torch.float64)
    for i in range(3):
        if b[i + 1] > b[i]:
            ref[b[i]:b[i + 1]] = F.layer_norm(x32[b[i]:b[i + 1]].double(), (N,), lw[i].double(), lb[i].double(), eps)
    if fp8:
        sb = torch.from_numpy(got["xn_scale"].cpu().numpy()[sidx])
        diff = (sb.int() - scale_bytes(ref.float().abs().reshape(M, N // 32, 32).amax(2)).int()).abs()
        assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
        back = dequant(got["xn8"].cpu().view(E4M3), sb)
        blockmax = ref.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
        assert float(((back - ref).abs() / blockmax).max()) <= 2.0 ** -4 * 1.01
    else:
        err = (got["xn16"].cpu().double() - ref).abs()
        tol = OUT_EPS[dtype] * ref.abs().clamp_min(1.0) + 2e-5 * ref.abs().clamp_min(1.0)
        assert bool((err <= 1.01 * tol).all()), float((err / tol).max())
        assert rel_l2(got["xn16"].float().cpu(), ref) < OUT_EPS[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", EMBED_IDS)
def test_patch_embed(dtype, cfg):
    """2 windows of 65 patches, C = 132: the cls rows keep the fill; bound: test_gpu_layout.py test_patch_embed (1e-4 of rms)"""
    windows, P, Cc = 2, 65, 132
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    g = torch.Generator().manual_seed(windows + P + Cc)
    patches = torch.randn(windows * P, 768, generator=g).to(T)
    w = (torch.randn(Cc, 768, generator=g) / math.sqrt(768)).to(T)
    bias, pos = torch.randn(Cc, generator=g), torch.randn(P + 1, Cc, generator=g)
    tile(256 * 768 * 2)  # (the 352-row tile takes no patch embed)

    def build(fs):
        Pt, Wt, b, ps = fs.inp(patches), fs.inp(w), fs.inp(bias), fs.inp(pos)
        tok = fs.out(F32, (windows, P + 1, Cc))
        return (lambda: ctx.lib.me_op_patch_embed(ctx.handle, p(Pt), windows, P, Cc, p(Wt), p(b), p(ps), p(tok), cfg)), {"tokens": tok}

    written = torch.ones(windows, P + 1, dtype=torch.bool)
    written[:, 0] = False
    tok = settle(run_both(ctx, build), masks={"tokens": written})["tokens"].cpu()
    ref = R.patch_embed_tokens(patches, w, bias, pos, torch.zeros(Cc), P)
    assert max_abs_rel(tok[:, 1:], ref[:, 1:]) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------------
def conv_case(ctx, dtype, geom, cfg, seed):
    """me_op_conv2d and me_op_conv2d_forms with 1, 2 and 3 output parts on one problem (test_gpu_split_forms.py conv_problem: both
    f32 residual inputs), bordered 16-bit output with ReLU beside the f32 output.  Bounds: test_gpu_ops.py test_conv2d (3e-5 /
    24 roundings of rms) for me_op_conv2d, test_gpu_split_forms.py check_16bit with CONV_BOUND for the forms."""
    T = TORCH16[dtype]
    B, H, Wd, Cin, Cout, k, s = geom
    pr = SF.conv_problem(T, B, H, Wd, Cin, Cout, k, s, 1, seed, res=2)
    Ho, Wo = pr["Ho"], pr["Wo"]
    M = B * Ho * Wo
    ref, ref16 = pr["ref"], pr["ref"].clamp_min(0.0)
    tile(18 * (Wd + 2) * Cin * 2)       # the rows of the input one tile spans: an 18-row halo at the most
    inner = torch.zeros(B, Ho + 2, Wo + 2, dtype=torch.bool)
    inner[:, 1:-1, 1:-1] = True
    for parts in (0, 1, 2, 3):                  # 0: me_op_conv2d

        def build(fs):
            xb, w, b = fs.inp(pr["xb"]), fs.inp(pr["w"]), fs.inp(pr["bias"])
            r1, r2 = fs.inp(pr["res"][0]), fs.inp(pr["res"][1])
            o32, o16 = fs.out(F32, (M, Cout)), fs.out(T, (B, Ho + 2, Wo + 2, max(parts, 1) * Cout))
            if parts == 0:
                return (lambda: ctx.lib.me_op_conv2d(ctx.handle, p(xb), B, H, Wd, Cin, p(w), Cout, k, s, p(b), p(r1), p(r2), p(o32), p(o16),
                                                     1, 2, 0, cfg)), {"out32": o32, "out16": o16}
            return (lambda: ctx.lib.me_op_conv2d_forms(ctx.handle, p(xb), B, H, Wd, Cin, p(w), Cout, k, s, p(b), p(r1), p(r2), p(o32),
                                                       p(o16), 1, parts, 2, 0, cfg)), {"out32": o32, "out16": o16}

        got = settle(run_both(ctx, build), masks={"out16": inner})
        tag = f"conv {dtype} {geom} cfg {cfg} parts {parts}"
        assert max_abs_rel(got["out32"].cpu(), ref) < 3e-5, tag
        px = got["out16"][:, 1:-1, 1:-1].reshape(M, -1)
        if parts == 0:
            assert max_abs_rel(px.float().cpu(), ref16) < 6 * OUT_EPS[dtype] * 4, tag
        else:
            SF.check_16bit(px, ref16, T, parts, SF.CONV_BOUND, True, got["out32"], tag)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", CONV_IDS)
@pytest.mark.parametrize("geom", [(2, 5, 7, 64, 36, 3, 1), (1, 6, 10, 128, 36, 3, 2), (2, 5, 7, 64, 36, 1, 1)])
def test_conv2d(dtype, cfg, geom):
    """maps smaller than any tile, odd sizes, Cout off the 8-element store: 3x3, 3x3 stride 2, 1x1, on every implicit-GEMM tile"""
    conv_case(ctx_for("tiny", dtype), dtype, geom, cfg, sum(geom))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,geom", [(TC.CFG_HALO, (2, 16, 16, 64, 256, 3, 1)), (TC.CFG_HALO12, (1, 12, 16, 64, 256, 3, 1)),
                                      (TC.CFG_HALO_N128, (1, 16, 16, 64, 128, 3, 1))])
def test_conv2d_halo_tiles(dtype, cfg, geom):
    """one tile of each halo configuration: its 18- (14-) row halo starts a row above and ends a row below the image"""
    assert (geom[1], geom[4]) == TC.HALO_IDS[cfg]
    conv_case(ctx_for("tiny", dtype), dtype, geom, cfg, sum(geom))


def convt_operands(dtype, B, H, Wd, Cin, Cout, seed):
    T = TORCH16[dtype]
    tile(352 * Cin * 2)                     # one row tile of the operand rows
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B * H * Wd, Cin, generator=g).to(T)
    w = (torch.randn(Cin, Cout, 2, 2, generator=g) / math.sqrt(Cin)).to(T)
    bias = torch.randn(Cout, generator=g)
    return a, w, bias


def convt_ref(a, w, bias, B, H, Wd):
    """fp64 ConvTranspose2d(2, 2, stride 2) of NHWC rows a [B * H * W][Cin] -> [B][2H][2W][Cout]"""
    x = R.nhwc_to_nchw(a.double().reshape(B, H, Wd, -1))
    return R.nchw_to_nhwc(F.conv_transpose2d(x, w.double(), bias.double() if bias is not None else None, stride=2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", CONVT_IDS)
def test_conv_transpose(dtype, cfg):
    """(2, 3, 5, 128, 36): f32 and bordered 16-bit output.  Bounds: test_gpu_ops.py test_conv_transpose.  Cout = 36 = 8 k + 4:
    every other sub-pixel boundary falls inside an 8-column granule of the epilogue, which must place the granule's halves
    separately (this is the case at which the fences found it placing them together: DESIGN.md 4.43)."""
    B, H, Wd, Cin, Cout = 2, 3, 5, 128, 36
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, w, bias = convt_operands(dtype, B, H, Wd, Cin, Cout, 99)
    wp = pack_convt(w.float()).to(T)

    def build(fs):
        A, Wt, b = fs.inp(a), fs.inp(wp), fs.inp(bias)
        o32, o16 = fs.out(F32, (B, 2 * H, 2 * Wd, Cout)), fs.out(T, (B, 2 * H + 2, 2 * Wd + 2, Cout))
        return (lambda: ctx.lib.me_op_conv_transpose2x2(ctx.handle, p(A), B, H, Wd, Cin, p(Wt), Cout, p(b), p(o32), p(o16), 1, cfg)), \
            {"out32": o32, "out16": o16}

    inner = torch.zeros(B, 2 * H + 2, 2 * Wd + 2, dtype=torch.bool)
    inner[:, 1:-1, 1:-1] = True
    got = settle(run_both(ctx, build), masks={"out16": inner})
    ref = convt_ref(a, w, bias, B, H, Wd)
    assert max_abs_rel(got["out32"].cpu(), ref) < 2e-5
    assert max_abs_rel(got["out16"][:, 1:-1, 1:-1].float().cpu(), ref) < 6 * OUT_EPS[dtype] * 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", CONVT_IDS)
@pytest.mark.parametrize("form", ["plain", "split", "slice", "wrap"])
def test_conv_transpose_forms(dtype, cfg, form):
    """(2, 3, 5, 128, 36), Cout = 8 k + 4 as in test_conv_transpose.  plain: f32 + bordered ReLU'd 16-bit; split: bordered
    [hi | lo] with the lo part 40 channels behind the hi part in pixels 80 channels apart (pixel_stride and lo_off are taken in
    multiples of 8: channels 36 .. 39 and 76 .. 79 of every pixel keep the fill); slice: channels 40 .. 75 of pixels 120 channels
    apart, whose other channels keep the fill; wrap: rows stored 64 channels wide, channels 64 .. 127 read from the row's start.
    Bounds: test_gpu_split_forms.py convt_case (LIN_BOUND, check_16bit)."""
    B, H, Wd, Cin, Cout = 2, 3, 5, 128, 36
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    a, w, bias = convt_operands(dtype, B, H, Wd, Cin, Cout, 51)
    wp = pack_convt(w.float()).to(T)
    wrap = 64 if form == "wrap" else 0
    stored = a[:, :wrap].contiguous() if wrap else a
    full = torch.cat([stored, stored], dim=1) if wrap else a
    split = 1 if form == "split" else 0
    border = 0 if form == "slice" else 1
    relu = form in ("plain", "wrap")
    stride_px = {"slice": 120, "split": 80}.get(form, Cout)
    lo_off = 40 if split else 0
    c0 = 40 if form == "slice" else 0
    oH, oW = 2 * H + 2 * border, 2 * Wd + 2 * border

    def build(fs):
        A, Wt, b = fs.inp(stored), fs.inp(wp), fs.inp(bias)
        o32, o16 = fs.out(F32, (B, 2 * H, 2 * Wd, Cout)), fs.out(T, (B, oH, oW, stride_px))
        args = (p(Wt), Cout, p(b), p(o32), p(o16, c0 * 2), border, 2 if relu else 0, split, stride_px if stride_px != Cout else 0, lo_off, cfg)
        if wrap:
            return (lambda: ctx.lib.me_op_conv_transpose2x2_forms_wrap(ctx.handle, p(A), B, H, Wd, Cin, wrap, *args)), {"out32": o32, "out16": o16}
        return (lambda: ctx.lib.me_op_conv_transpose2x2_forms(ctx.handle, p(A), B, H, Wd, Cin, *args)), {"out32": o32, "out16": o16}

    written = torch.zeros(B, oH, oW, stride_px, dtype=torch.bool)
    inner = written[:, 1:-1, 1:-1] if border else written
    inner[..., c0:c0 + Cout] = True
    if split:
        inner[..., lo_off:lo_off + Cout] = True
    got = settle(run_both(ctx, build), masks={"out16": written})
    ref = convt_ref(full, w, bias, B, H, Wd).reshape(-1, Cout)
    assert max_abs_rel(got["out32"].reshape(-1, Cout).cpu(), ref) < SF.LIN_BOUND
    core = got["out16"][:, 1:-1, 1:-1] if border else got["out16"]
    px = core[..., c0:c0 + Cout].reshape(-1, Cout)
    if split:
        px = torch.cat([px, core[..., lo_off:lo_off + Cout].reshape(-1, Cout)], dim=1)
    SF.check_16bit(px, ref.clamp_min(0.0) if relu else ref, T, 2 if split else 1, SF.LIN_BOUND, relu, got["out32"].reshape(-1, Cout),
                   f"convt {form} {dtype} cfg {cfg}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_transpose_pair(dtype):
    """The smallest case of test_gpu_convt_pair.py ("one_tile": 8 x 8, 128 + 192 -> 64, tile 0) from its own operand builders.
    Bounds: out32 within BOUND of the fp64 sum (test_pair_on_random_operands); out16 is set a's ReLU'd 16-bit output, held as
    me_op_conv_transpose2x2_forms' is (test_gpu_split_forms.py check_16bit with LIN_BOUND)."""
    B, H, Wd, Ka, pa, Kb, pb, Cout, cap = CP.SHAPES["one_tile"]
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(352 * max(Ka, Kb) * 2)
    M = B * H * Wd
    g = torch.Generator().manual_seed(1234)
    Aa, Ab = CP.operand(g, M, Ka, pa, T, False), CP.operand(g, M, Kb, pb, T, False)
    Wa, Wb = CP.weights(g, Ka, Cout, T, False), CP.weights(g, Kb, Cout, T, False)
    bias = torch.randn(Cout, generator=g)

    def build(fs):
        a_, wa, b_, wb, bb = fs.inp(Aa), fs.inp(Wa), fs.inp(Ab), fs.inp(Wb), fs.inp(bias)
        o32, o16 = fs.out(F32, (B, 2 * H, 2 * Wd, Cout)), fs.out(T, (B, 2 * H + 2, 2 * Wd + 2, Cout))
        return (lambda: ctx.lib.me_op_conv_transpose2x2_pair(ctx.handle, B, H, Wd, Cout, p(a_), Ka, p(wa), p(b_), Kb, 0, p(wb), p(bb), p(o32),
                                                             p(o16), 1, CP.RELU, cap, 0)), {"out32": o32, "out16": o16}

    inner = torch.zeros(B, 2 * H + 2, 2 * Wd + 2, dtype=torch.bool)
    inner[:, 1:-1, 1:-1] = True
    got = settle(run_both(ctx, build), masks={"out16": inner})
    first = CP.shuffle(Aa.double() @ Wa.double().T, B, H, Wd, Cout)
    ref = first + CP.shuffle(Ab.double() @ Wb.double().T + bias.double().repeat(4), B, H, Wd, Cout)
    assert max_abs_rel(got["out32"].cpu(), ref) < CP.BOUND
    SF.check_16bit(got["out16"][:, 1:-1, 1:-1].reshape(-1, Cout), first.reshape(-1, Cout).clamp_min(0.0), T, 1, SF.LIN_BOUND, True, None,
                   f"pair {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom,cfg", [((1, 12, 16, 128, 32), -1), ((2, 5, 7, 64, 32), -1), ((2, 5, 7, 64, 32), 2)])
def test_head_final(dtype, geom, cfg):
    """One tile of the halo kernel (the model's channels) and a map smaller than a tile on the implicit-GEMM tile, both with a
    per-image f_norm and a clamp.  Bound: test_gpu_ops.py test_head_final (2e-5 of the largest value)."""
    B, H, Wd, Cin, Cmid = geom
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    g = torch.Generator().manual_seed(H * Wd + Cin)
    x = torch.randn(B, Cin, H, Wd, generator=g)
    w = (torch.randn(Cmid, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(T)
    bias = torch.randn(Cmid, generator=g) * 0.3
    w2 = torch.randn(Cmid, generator=g) / math.sqrt(Cmid)
    b2 = torch.tensor([0.4])
    f_norm = 0.5 + torch.rand(B, generator=g)
    lo, hi = 0.2, 1.5
    xb = torch.zeros(B, H + 2, Wd + 2, Cin, dtype=T)
    xb[:, 1:-1, 1:-1] = R.nchw_to_nhwc(x).to(T)
    wp = pack_conv(w.float()).to(T)
    tile(14 * (Wd + 2) * Cin * 2)           # the 12 + 2 rows of one halo tile

    def build(fs):
        X, Wt, b, W2, B2, fn = fs.inp(xb), fs.inp(wp), fs.inp(bias), fs.inp(w2), fs.inp(b2), fs.inp(f_norm)
        o = fs.out(F32, (B, H, Wd))
        return (lambda: ctx.lib.me_op_head_final(ctx.handle, p(X), B, H, Wd, Cin, p(Wt), Cmid, p(b), p(W2), p(B2), p(fn), lo, hi, p(o), cfg)), \
            {"out32": o}

    got = settle(run_both(ctx, build))["out32"].cpu().double()
    mid = F.relu(F.conv2d(R.nhwc_to_nchw(xb[:, 1:-1, 1:-1].double()), w.double(), bias.double(), padding=1))
    ref = F.relu((mid * w2.double().view(1, Cmid, 1, 1)).sum(1) + b2.double())
    ref = (ref / f_norm.double().view(B, 1, 1)).clamp(lo, hi)
    assert float((got - ref).abs().max()) < 2e-5 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
ATT_CASES = [(1, 1, 1), (2, 65, 1), (3, 130, 2), (1, 577, 2)]      # (windows, tokens, heads)
_ATT = {}


def att_problem(dtype, windows, tokens, heads, prescaled):
    """(qkv [windows * tokens][3 C] in the 16-bit type, fp64 softmax attention of it), made once and left unchanged"""
    key = (dtype, windows, tokens, heads, prescaled)
    tile(192 * 3 * heads * 64 * 2)  # the 6 x 32 query rows of a workgroup (a key tile is 64 rows)
    if key not in _ATT:
        Cc = heads * 64
        g = torch.Generator().manual_seed(tokens + 3 * heads + prescaled)
        x = torch.randn(windows * tokens, 3 * Cc, generator=g) * 1.5
        if prescaled:
            x[:, :Cc] *= QSCALE
        qkv = x.to(TORCH16[dtype])
        xx = qkv.cuda().double().reshape(windows, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = (xx[0] @ xx[1].transpose(3, 2)) * (math.log(2.0) if prescaled else 0.125)
        ref = (torch.softmax(s, dim=3) @ xx[2]).transpose(1, 2).reshape(windows * tokens, Cc).cpu()
        _ATT[key] = (qkv, ref)
    return _ATT[key]


def att_bounds(got, ref, dtype):
    """test_gpu_ops.py test_attention / test_attention_prescaled"""
    assert max_err_over_max(got.float().cpu(), ref) < 2 * OUT_EPS[dtype]
    assert rel_l2(got.float().cpu(), ref) < 1.5 * OUT_EPS[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prescaled", [0, 1])
@pytest.mark.parametrize("windows,tokens,heads", ATT_CASES)
def test_attention(dtype, prescaled, windows, tokens, heads):
    """one token; one key past a 64-key tile; two query blocks and two heads; the model's 577.  The kernels clamp their loads at
    the last row of the window: a clamp one row off reads the fence."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    qkv, ref = att_problem(dtype, windows, tokens, heads, prescaled)
    fn = "me_op_attention_prescaled" if prescaled else "me_op_attention"

    def build(fs):
        q = fs.inp(qkv)
        o = fs.out(T, (windows * tokens, heads * 64))
        return (lambda: getattr(ctx.lib, fn)(ctx.handle, p(q), p(o), windows, tokens, heads)), {"out16": o}

    att_bounds(settle(run_both(ctx, build))["out16"], ref, dtype)


def fp8_rows_equal(got8, got_scale, sidx, want16):
    """test_gpu_row_segments.py _fp8_output_check: bytes and scale bytes are the MX rule on the 16-bit output, code for code"""
    q_ref, sb_ref = quantize_ref(want16.float().cpu())
    assert bool((got8.cpu().view(E4M3).float() == q_ref.float()).all())
    assert np.array_equal(got_scale.cpu().numpy()[sidx], sb_ref.numpy())


@pytest.mark.parametrize("windows,tokens", [(w, t) for w, t, _ in ATT_CASES])
def test_attention_fp8(windows, tokens):
    """two heads throughout (the fp8 forms take even head counts).  The bytes are the MX rule applied to me_op_attention's 16-bit
    output of the same input (test_gpu_fp8.py test_attention_fp8_output_equals_quantised_16bit_output), itself fenced here."""
    heads, Cc, rows = 2, 128, windows * tokens
    ctx = ctx_for("tiny", "f16")
    qkv, ref = att_problem("f16", windows, tokens, heads, 0)
    smask, sidx = act_scale_mask(rows, Cc)

    def build16(fs):
        q = fs.inp(qkv)
        o = fs.out(torch.float16, (rows, Cc))
        return (lambda: ctx.lib.me_op_attention(ctx.handle, p(q), p(o), windows, tokens, heads)), {"out16": o}

    def build8(fs):
        q = fs.inp(qkv)
        o8, os_ = fs.out(U8, (rows, Cc)), fs.out(U8, (smask.numel(),))
        return (lambda: ctx.lib.me_op_attention_fp8(ctx.handle, p(q), p(o8), p(os_), windows, tokens, heads)), {"out8": o8, "scale": os_}

    out16 = settle(run_both(ctx, build16))["out16"]
    att_bounds(out16, ref, "f16")
    got = settle(run_both(ctx, build8), masks={"scale": smask})
    fp8_rows_equal(got["out8"], got["scale"], sidx, out16)


def gapped_layout(windows, tokens):
    """a row space with rows of no window between and behind the segments: three segments where there are three windows, two
    otherwise (the second empty when there is one window)"""
    if windows >= 3:
        seg1 = tokens + 3
        seg2 = seg1 + tokens + 5
        return RS.Layout(tokens, windows, seg1, seg2, 1, 1, seg2 + (windows - 2) * tokens + 2)
    win0 = 1
    seg1 = tokens + 3
    return RS.Layout(tokens, windows, seg1, 0, win0, windows - win0, seg1 + (windows - win0) * tokens + 2)


@pytest.mark.parametrize("dtype,fp8", DTYPE_FORMS)
@pytest.mark.parametrize("prescaled", [0, 1])
@pytest.mark.parametrize("windows,tokens,heads", ATT_CASES)
def test_attention_segments(dtype, fp8, prescaled, windows, tokens, heads):
    """The windows of test_attention in a segmented row space with gap rows: the gap rows of the INPUT hold the fill (NaN keys
    under 0xFF), those of the output must still hold it afterwards.  out16 against fp64 within test_attention's bounds; out8 is
    the MX rule on that out16, code for code (test_gpu_row_segments.py)."""
    form = "out8" if fp8 else "out16"
    if fp8:
        heads = 2           # the fp8 forms take even head counts
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    Cc = heads * 64
    lay = gapped_layout(windows, tokens)
    qkv, ref = att_problem(dtype, windows, tokens, heads, prescaled)
    index = torch.tensor([r0 + t for r0 in RS.window_rows(lay) for t in range(tokens)])
    rows_written = torch.zeros(lay.rows_total, dtype=torch.bool)
    rows_written[index] = True
    assert int((~rows_written).sum()) >= 5
    if fp8:                 # the scale bytes of the windows' rows alone are written
        smask, sidx = act_scale_mask(lay.rows_total, Cc)
        smask[:] = False
        smask[torch.from_numpy(sidx[index.numpy()].ravel())] = True

    def build(fs, want8):
        spread = torch.empty(lay.rows_total, 3 * Cc, dtype=T)
        spread.view(torch.int16).fill_(-1 if fs.fill else 0)          # the gap rows of the input hold the fill
        spread[index] = qkv
        q = fs.inp(spread)
        if want8:
            o8, os_ = fs.out(U8, (lay.rows_total, Cc)), fs.out(U8, (smask.numel(),))
            outs, args = {"out8": o8, "scale": os_}, (None, p(o8), p(os_))
        else:
            o = fs.out(T, (lay.rows_total, Cc))
            outs, args = {"out16": o}, (p(o), None, None)
        return (lambda: ctx.lib.me_op_attention_segments(ctx.handle, p(q), *args, windows, tokens, heads, prescaled, lay.rows_total,
                                                         lay.seg1, lay.seg2, lay.win0, lay.win1)), outs

    out16 = settle(run_both(ctx, lambda fs: build(fs, False)), masks={"out16": rows_written})["out16"][index.cuda()]
    att_bounds(out16, ref, dtype)
    if form == "out8":
        got = settle(run_both(ctx, lambda fs: build(fs, True)), masks={"out8": rows_written, "scale": smask})
        fp8_rows_equal(got["out8"][index.cuda()], got["scale"], sidx[index.numpy()], out16)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def ln_operands(rows, dim, sets=1):
    """x as in test_gpu_ops.py test_layernorm; up to three weight sets of its magnitude (|w| near 1, so that its bounds hold) and
    far enough apart that a row on another segment's set is wrong by O(1)"""
    tile(4 * dim * 4)                       # the four rows of a workgroup
    g = torch.Generator().manual_seed(rows + dim)
    x = torch.randn(rows, dim, generator=g) * 3 + 0.5
    ws = [wm + 0.02 * torch.randn(dim, generator=g) for wm in (1.0, -1.0, 0.9)[:sets]]
    bs = [bm + 0.02 * torch.randn(dim, generator=g) for bm in (0.0, 0.5, -0.5)[:sets]]
    return x, ws, bs


def ln_fp8_bounds(got8, got_scale, sidx, ref):
    """test_gpu_fp8.py _layernorm_fp8_case"""
    rows, dim = ref.shape
    sb = torch.from_numpy(got_scale.cpu().numpy()[sidx])
    diff = (sb.int() - scale_bytes(ref.float().abs().reshape(rows, dim // 32, 32).amax(2)).int()).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    back = dequant(got8.cpu().view(E4M3), sb)
    blockmax = ref.abs().reshape(rows, dim // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(rows, dim)
    assert float(((back - ref).abs() / blockmax).max()) <= 2.0 ** -4 * 1.01


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("dim", [64, 1024])
def test_layernorm(dtype, rows, dim):
    """one row, and a row count that ends inside a workgroup's four rows; bounds: test_gpu_ops.py test_layernorm"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    x, ws, bs = ln_operands(rows, dim)

    def build(fs):
        X, Wt, b = fs.inp(x), fs.inp(ws[0]), fs.inp(bs[0])
        y16, y32 = fs.out(T, (rows, dim)), fs.out(F32, (rows, dim))
        return (lambda: ctx.lib.me_op_layernorm(ctx.handle, p(X), p(Wt), p(b), p(y16), p(y32), rows, dim, 1e-5)), {"y16": y16, "y32": y32}

    got = settle(run_both(ctx, build))
    ref = F.layer_norm(x.double(), (dim,), ws[0].double(), bs[0].double(), 1e-5)
    assert float((got["y32"].cpu().double() - ref).abs().max()) < 2e-5
    assert float((got["y16"].cpu().double() - ref).abs().max()) < 4 * OUT_EPS[dtype] * 2


@pytest.mark.parametrize("rows", [1, 5])
def test_layernorm_fp8(rows):
    """dim 256; the scale bytes of the rows behind `rows` in the 128-row tile are not written"""
    dim = 256
    ctx = ctx_for("tiny", "f16")
    x, ws, bs = ln_operands(rows, dim)
    smask, sidx = act_scale_mask(rows, dim)

    def build(fs):
        X, Wt, b = fs.inp(x), fs.inp(ws[0]), fs.inp(bs[0])
        y8, ys = fs.out(U8, (rows, dim)), fs.out(U8, (smask.numel(),))
        return (lambda: ctx.lib.me_op_layernorm_fp8(ctx.handle, p(X), p(Wt), p(b), p(y8), p(ys), rows, dim, 1e-5)), {"y8": y8, "yscale": ys}

    got = settle(run_both(ctx, build), masks={"yscale": smask})
    ln_fp8_bounds(got["y8"], got["yscale"], sidx, F.layer_norm(x.double(), (dim,), ws[0].double(), bs[0].double(), 1e-5))


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("dtype,dim,fp8", [("f16", 64, 0), ("bf16", 64, 0), ("f16", 1024, 0), ("bf16", 1024, 0), ("f16", 256, 1)])
def test_layernorm_segments(dtype, rows, dim, fp8):
    """five rows in segments of 2 | 2 | 1 with three weight sets (one row: one segment).  test_gpu_row_segments.py holds the
    segmented launch bit for bit to me_op_layernorm / me_op_layernorm_fp8 per segment; their bounds against fp64 are used here."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    seg1, seg2 = (2, 4) if rows == 5 else (0, 0)
    nset = 3 if seg1 else 1
    x, ws, bs = ln_operands(rows, dim, sets=nset)
    smask, sidx = act_scale_mask(rows, dim)

    def build(fs):
        X = fs.inp(x)
        Ws, Bs = [fs.inp(w) for w in ws] + [None] * (3 - nset), [fs.inp(b) for b in bs] + [None] * (3 - nset)
        if fp8:
            y8, ys = fs.out(U8, (rows, dim)), fs.out(U8, (smask.numel(),))
            outs, args = {"y8": y8, "yscale": ys}, (None, None, p(y8), p(ys))
        else:
            y16, y32 = fs.out(T, (rows, dim)), fs.out(F32, (rows, dim))
            outs, args = {"y16": y16, "y32": y32}, (p(y16), p(y32), None, None)
        return (lambda: ctx.lib.me_op_layernorm_segments(ctx.handle, p(X), arr3(Ws), arr3(Bs), seg1, seg2, *args, rows, dim, 1e-5)), outs

    got = settle(run_both(ctx, build), masks={"yscale": smask})
    b = seg_bounds(rows, seg1, seg2)
    ref = torch.cat([F.layer_norm(x[b[i]:b[i + 1]].double(), (dim,), ws[i].double(), bs[i].double(), 1e-5)
                     for i in range(3) if b[i + 1] > b[i]])
    if fp8:
        ln_fp8_bounds(got["y8"], got["yscale"], sidx, ref)
    else:
        assert float((got["y32"].cpu().double() - ref).abs().max()) < 2e-5
        assert float((got["y16"].cpu().double() - ref).abs().max()) < 4 * OUT_EPS[dtype] * 2


# ---------------------------------------------------------------------------------------------------------------------
# fp8
# ---------------------------------------------------------------------------------------------------------------------
def wgt_scale_index(rows, K):
    """csrc/mx_fp8.h w_scale_index as test_gpu_fp8.py _scale_table states it"""
    nt = rows // 64
    r = np.arange(rows, dtype=np.int64)[:, None]
    kb = np.arange(K // 32, dtype=np.int64)[None, :]
    return (((kb >> 2) * nt + (r >> 6)) * 64 + (kb & 3) * 16 + (r & 15)) * 4 + ((r & 63) >> 4)


@pytest.mark.parametrize("rows,K,weight_layout", [(65, 256, 0), (64, 256, 1)])
def test_quantize_fp8(rows, K, weight_layout):
    """one row past a 64-row group in the activation layout (63 rows of the 128-row scale tile are not written); one group of
    the weight layout.  Exact: test_gpu_fp8.py test_quantizer_is_the_mx_rule."""
    ctx = ctx_for("tiny", "f16")
    tile(128 * K * 2)  # the rows of one scale tile
    g = torch.Generator().manual_seed(3 + weight_layout)
    x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 3)
    x[5, 32:64] = 0.0
    x[7, 0] = 60000.0
    x16 = x.half()
    if weight_layout:
        sidx = wgt_scale_index(rows, K)
        smask = torch.ones(rows * K // 32, dtype=torch.bool)
    else:
        smask, sidx = act_scale_mask(rows, K)

    def build(fs):
        X = fs.inp(x16)
        d8, sc = fs.out(U8, (rows, K)), fs.out(U8, (smask.numel(),))
        return (lambda: ctx.lib.me_op_quantize_fp8(ctx.handle, p(X), rows, K, weight_layout, p(d8), p(sc))), {"dst8": d8, "scales": sc}

    got = settle(run_both(ctx, build), masks={"scales": smask})
    q_ref, sb_ref = quantize_ref(x16.float())
    assert torch.equal(got["dst8"].cpu().view(E4M3).float(), q_ref.float())
    assert np.array_equal(got["scales"].cpu().numpy()[sidx], sb_ref.numpy())
    for r, kb in ((0, 0), (rows - 1, K // 32 - 1), (17, 3)):        # the numpy formulas are me_op_scale_index
        assert int(sidx[r, kb]) == ctx.lib.me_op_scale_index(r, kb, rows, weight_layout)


_FP8 = {}


def fp8_problem(M, N, K, nseg, seed):
    """test_gpu_fp8.py _fp8_problem, read back to the host: quantised operands (bytes and packed scales as the library's own
    quantiser lays them out, in ordinary tensors) and the dequantised f64 matrices"""
    key = (M, N, K, nseg, seed)
    tile(352 * K)                           # one row tile of the tallest configuration, e4m3 bytes
    if key not in _FP8:
        ctx = ctx_for("tiny", "f16")
        a8, asc, A, wsets = F8._fp8_problem(ctx, torch.Generator().manual_seed(seed), M, N, K, nseg)
        _FP8[key] = (a8.cpu(), asc.cpu(), A.cpu(), [tuple(t.cpu() for t in ws) for ws in wsets[:nseg]])
    return _FP8[key]


@pytest.mark.parametrize("form", ["out16", "out8", "resid"])
def test_linear_fp8(form):
    """(256, 256, 256), the three output forms; bounds: test_gpu_fp8.py test_linear_fp8_against_dequantised_operands"""
    M = N = K = 256
    ctx = ctx_for("tiny", "f16")
    a8, asc, A, wsets = fp8_problem(M, N, K, 1, 11)
    w8, wsc, Wd, bias, gamma = wsets[0]
    x0 = torch.randn(M, N, generator=torch.Generator().manual_seed(12))
    smask, sidx = act_scale_mask(M, N)

    def build(fs):
        ops = (p(fs.inp(a8)), p(fs.inp(asc)), p(fs.inp(w8)), p(fs.inp(wsc)), p(fs.inp(bias)))
        if form == "out16":
            o = fs.out(torch.float16, (M, N))
            return (lambda: ctx.lib.me_op_linear_fp8(ctx.handle, M, N, K, *ops, p(o), None, None, None, None)), {"out16": o}
        if form == "out8":
            o8, os_ = fs.out(U8, (M, N)), fs.out(U8, (smask.numel(),))
            return (lambda: ctx.lib.me_op_linear_fp8(ctx.handle, M, N, K, *ops, None, p(o8), p(os_), None, None)), {"out8": o8, "scale": os_}
        G, X = fs.inp(gamma), fs.inout(x0)
        return (lambda: ctx.lib.me_op_linear_fp8(ctx.handle, M, N, K, *ops, None, None, None, p(G), p(X))), {"x32": X}

    got = settle(run_both(ctx, build))
    ref = A @ Wd.T + bias.double()
    if form == "out16":
        err = (got["out16"].cpu().double() - ref).abs()
        assert float((err / (ref.abs() * 2.0 ** -11 + 1e-3 * ref.abs().mean())).max()) < 1.6
    elif form == "resid":
        want = x0.double() + gamma.double() * ref
        assert float((got["x32"].cpu().double() - want).abs().max() / want.abs().max()) < 3e-5
    else:
        act = F.gelu(ref)
        _, sb_ref = quantize_ref(act.float())
        sb = torch.from_numpy(got["scale"].cpu().numpy()[sidx])
        diff = (sb.int() - sb_ref.int()).abs()
        assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
        back = dequant(got["out8"].cpu().view(E4M3), sb)
        blockmax = act.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
        assert float(((back - act).abs() / blockmax.clamp_min(1e-30)).max()) <= 2.0 ** -4 * 1.01 + 1e-6


@pytest.mark.parametrize("form", ["out16", "out8", "resid"])
def test_linear_fp8_segments(form):
    """M = 768 in segments 256 | 512 with their own weights, scales, bias and gamma.  Bounds: test_gpu_fp8.py
    test_linear_fp8_at_the_step_shapes_with_cold_caches (per element, no element may miss)."""
    M, N, K, seg1, seg2 = 768, 256, 256, 256, 512
    ctx = ctx_for("tiny", "f16")
    a8, asc, A, wsets = fp8_problem(M, N, K, 3, 21)
    x0 = torch.randn(M, N, generator=torch.Generator().manual_seed(22))
    smask, sidx = act_scale_mask(M, N)

    def build(fs):
        A8, AS = fs.inp(a8), fs.inp(asc)
        W8, WS, BI, GA = ([fs.inp(ws[i]) for ws in wsets] for i in (0, 1, 3, 4))
        head = (ctx.handle, M, N, K, p(A8), p(AS), seg1, seg2, arr3(W8), arr3(WS), arr3(BI))
        if form == "out16":
            o = fs.out(torch.float16, (M, N))
            return (lambda: ctx.lib.me_op_linear_fp8_segments(*head, None, p(o), None, None, None)), {"out16": o}
        if form == "out8":
            o8, os_ = fs.out(U8, (M, N)), fs.out(U8, (smask.numel(),))
            return (lambda: ctx.lib.me_op_linear_fp8_segments(*head, None, None, p(o8), p(os_), None)), {"out8": o8, "scale": os_}
        X = fs.inout(x0)
        return (lambda: ctx.lib.me_op_linear_fp8_segments(*head, arr3(GA), None, None, None, p(X))), {"x32": X}

    got = settle(run_both(ctx, build))
    ref = torch.cat([A[lo:hi] @ ws[2].T + ws[3].double() for (lo, hi), ws in zip(((0, seg1), (seg1, seg2), (seg2, M)), wsets)])
    if form == "out16":
        err = (got["out16"].cpu().double() - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -10 + 2e-3 * ref.abs().mean()).all())
    elif form == "resid":
        want = x0.double() + per_row([ws[4] for ws in wsets], M, seg1, seg2) * ref
        assert bool(((got["x32"].cpu().double() - want).abs() <= 1e-4 * want.abs().max()).all())
    else:
        act = F.gelu(ref)
        back = dequant(got["out8"].cpu().view(E4M3), torch.from_numpy(got["scale"].cpu().numpy()[sidx]))
        blockmax = act.abs().reshape(M, N // 32, 32).amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
        assert bool(((back - act).abs() <= blockmax * 2.0 ** -3 + 1e-6).all())


def test_linear_fp8_residual_layernorm():
    """(353, 256, 256): one row past the 352-row tile, which clamps its rows.  Bounds: test_gpu_fp8.py
    test_linear_fp8_residual_layernorm_fused."""
    M, N, K = 353, 256, 256
    ctx = ctx_for("tiny", "f16")
    a8, asc, A, wsets = fp8_problem(M, N, K, 1, 31)
    w8, wsc, Wd, bias, gamma = wsets[0]
    g = torch.Generator().manual_seed(32)
    lw, lb = 1.0 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    x0 = torch.randn(M, N, generator=g) * 2.0
    x0[:, 7] += 40.0
    x0[::3] *= 10.0
    smask, sidx = act_scale_mask(M, N)

    def build(fs):
        one = lambda t: arr3([fs.inp(t), None, None])
        A8, AS = fs.inp(a8), fs.inp(asc)
        X, o8, os_ = fs.inout(x0), fs.out(U8, (M, N)), fs.out(U8, (smask.numel(),))
        ptrs = (one(w8), one(wsc), one(bias), one(gamma), one(lw), one(lb))
        return (lambda: ctx.lib.me_op_linear_fp8_residual_layernorm(ctx.handle, M, N, K, p(A8), p(AS), 0, 0, *ptrs, 1e-5, p(X), p(o8),
                                                                    p(os_))), {"x32": X, "xn8": o8, "xn_scale": os_}

    ctx.status_flags()
    got = settle(run_both(ctx, build), masks={"xn_scale": smask})
    assert ctx.status_flags() == 0
    x32 = got["x32"].cpu().double()
    want = x0.double() + gamma.double() * (A @ Wd.T + bias.double())
    assert float((x32 - want).abs().max() / want.abs().max()) < 3e-5
    ln_fp8_bounds(got["xn8"], got["xn_scale"], sidx, F.layer_norm(x32, (N,), lw.double(), lb.double(), 1e-5))


# ---------------------------------------------------------------------------------------------------------------------
# layout and element-wise kernels: the smallest parameter tuple of each list of test_gpu_layout.py, bit for bit against
# layout_refs.py as there (bilinear and fov_final within the bounds written there)
# ---------------------------------------------------------------------------------------------------------------------
def same(got, want, zero_sign=True):
    LT.same_bits(got, want, zero_sign)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,out_size,planes,align", [(2, 5, 1, 1), (12, 3, 2, 0)])
def test_bilinear(dtype, n, out_size, planes, align):
    """bounds: test_gpu_layout.py _bilinear_check, restated from its own helpers"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(2 * n * 4)  # the two source rows of an output row
    src = LT.values((planes, n, n), n + out_size)
    src[src.abs() > 100] = 1.0

    def build(fs):
        S = fs.inp(src)
        o = fs.out(T, (planes, out_size, out_size))
        return (lambda: ctx.lib.me_op_bilinear(ctx.handle, p(S), p(o), planes, n, out_size, align)), {"dst16": o}

    got = settle(run_both(ctx, build))["dst16"].double().cpu()
    from oracle import depth_pro_oracle as O
    ref = O.interpolate_bilinear(src.double()[None], out_size, out_size, bool(align))[0]
    Rn, A = LT._neighbourhood(src.double(), out_size, align)
    slack = 2 * (2.0 ** -23 * (n - 1)) * Rn + 8 * 2.0 ** -24 * A if align else torch.full_like(ref, 4 * 2.0 ** -24 * float(src.abs().max()))
    assert bool(((got - ref).abs() <= LT._half_ulp(ref.abs() + slack, T) + slack).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify(dtype):
    """grid 8, one image; one window for me_op_patchify_windows"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(16 * 64 * 8 * 2)  # the 16 image rows of a row of patches, at the widest level
    grid, batch = 8, 1
    wp_, P = 16 * grid, grid * grid
    xs = [LT.values((batch, 3, s * wp_, s * wp_), grid * 10 + s).to(T) for s in (4, 2, 1)]

    def build(fs):
        X = [fs.inp(x) for x in xs]
        o = fs.out(T, (batch * 35 * P, 768))
        return (lambda: ctx.lib.me_op_patchify(ctx.handle, p(X[0]), p(X[1]), p(X[2]), p(o), batch, grid)), {"patches": o}

    same(settle(run_both(ctx, build))["patches"], R.patchify(xs[0], xs[1], xs[2], grid))
    win = LT.values((1, 3, wp_, wp_), grid + 1).to(T)

    def build_w(fs):
        X = fs.inp(win)
        o = fs.out(T, (P, 768))
        return (lambda: ctx.lib.me_op_patchify_windows(ctx.handle, p(X), p(o), 1, grid)), {"patches": o}

    same(settle(run_both(ctx, build_w))["patches"], R.patchify_windows(win, grid))


def test_cls_rows():
    """(1, 65, 128): row 0 is written, the 64 others keep the fill"""
    windows, tpw, dim = 1, 65, 128
    ctx = ctx_for("tiny", "f16")
    tile(dim * 4)
    cls, pos = LT.values((dim,), 1), LT.values((tpw, dim), 2)

    def build(fs):
        c, ps = fs.inp(cls), fs.inp(pos)
        tok = fs.out(F32, (windows, tpw, dim))
        return (lambda: ctx.lib.me_op_cls_rows(ctx.handle, p(tok), p(c), p(ps), windows, tpw, dim)), {"tokens": tok}

    written = torch.zeros(windows, tpw, dtype=torch.bool)
    written[:, 0] = True
    got = settle(run_both(ctx, build), masks={"tokens": written})["tokens"]
    same(got[:, 0], (cls + pos[0]).expand(windows, dim))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("source,split", [(32, 0), (32, 1), (16, 0)])
def test_merge(dtype, source, split):
    """(grid 8, batch 1, dim 64) over the four window geometries; f32 source, f32 source split into [hi | lo], 16-bit source"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(64 * 4)  # one token row
    grid, batch, dim = 8, 1, 64
    for gi, (wpi, win0, steps, padding) in enumerate(LT._merge_geometries(grid)):
        tok = LT.values((batch * wpi, grid * grid + 1, dim), 8000 + 10 * gi + source + split)
        if source == 16:
            tok = tok.to(T)
        ref = R.merge(tok, batch, wpi, win0, steps, padding, grid)
        want = R.split_pixels(ref, T) if split else ref.to(T)

        def build(fs):
            t = fs.inp(tok)
            o = fs.out(T, want.shape)
            return (lambda: ctx.lib.me_op_merge(ctx.handle, p(t) if source == 32 else None, p(t) if source == 16 else None, p(o), batch, wpi,
                                                win0, steps, padding, grid, dim, split)), {"dst16": o}

        same(settle(run_both(ctx, build))["dst16"], want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_changes(dtype):
    """(B, C, H, W) = (1, 37, 5, 7) and (B, H, W, C) = (1, 5, 7, 12): NCHW f32 -> NHWC in every 16-bit form (the border keeps the
    fill) with the f32 copy, back from 16 bit (an INPUT border of the fill: reading it would show) and from f32, and f32 NHWC
    into a bordered map"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(32 * 32 * 4)  # one transposing tile
    B, Cc, H, Wd = LT.MAPS[0]
    x = LT.values((B, Cc, H, Wd), B + Cc + H + Wd)
    nhwc = R.nchw_to_nhwc(x)
    inner = torch.zeros(B, H + 2, Wd + 2, dtype=torch.bool)
    inner[:, 1:-1, 1:-1] = True
    for border in (0, 1):
        for relu16 in (0, 1):
            for split in (0, 1):
                a = nhwc.clamp_min(0.0) if relu16 else nhwc
                w16 = R.split_pixels(a, T) if split else a.to(T)

                def build(fs):
                    X = fs.inp(x)
                    o32, o16 = fs.out(F32, nhwc.shape), fs.out(T, (B, H + 2 * border, Wd + 2 * border, w16.shape[-1]))
                    return (lambda: ctx.lib.me_op_nchw32_to_nhwc(ctx.handle, p(X), p(o32), p(o16), B, H, Wd, Cc, border, relu16, split)), \
                        {"dst32": o32, "dst16": o16}

                got = settle(run_both(ctx, build), masks={"dst16": inner} if border else None)
                same(got["dst16"][:, 1:-1, 1:-1] if border else got["dst16"], w16, zero_sign=not relu16)
                same(got["dst32"], nhwc)
    v = R.nchw_to_nhwc(LT.values((B, Cc, H, Wd), B + Cc + H + Wd + 1))
    for border in (0, 1):
        for split in (0, 1):
            src = R.split_pixels(v, T) if split else v.to(T)
            want = R.nhwc_to_nchw((src[..., :Cc].float() + src[..., Cc:].float()) if split else src.float())

            def build(fs):
                s = src
                if border:      # the input's border holds the fill, as the guards do
                    s = torch.empty(B, H + 2, Wd + 2, src.shape[-1], dtype=T)
                    s.view(torch.int16).fill_(-1 if fs.fill else 0)
                    s[:, 1:-1, 1:-1] = src
                S = fs.inp(s)
                o = fs.out(F32, (B, Cc, H, Wd))
                return (lambda: ctx.lib.me_op_nhwc16_to_nchw32(ctx.handle, p(S), p(o), B, H, Wd, Cc, border, split)), {"dst": o}

            same(settle(run_both(ctx, build))["dst"], want)

    def build32(fs):
        S = fs.inp(v)
        o = fs.out(F32, (B, Cc, H, Wd))
        return (lambda: ctx.lib.me_op_nhwc32_to_nchw32(ctx.handle, p(S), p(o), B, H, Wd, Cc)), {"dst": o}

    same(settle(run_both(ctx, build32))["dst"], R.nhwc_to_nchw(v))
    B, H, Wd, Cc = 1, 5, 7, 12
    u = LT.values((B, H, Wd, Cc), B + H + Wd + Cc + 2)
    inner = torch.zeros(B, H + 2, Wd + 2, dtype=torch.bool)
    inner[:, 1:-1, 1:-1] = True
    for relu in (0, 1):

        def build16b(fs):
            S = fs.inp(u)
            o = fs.out(T, (B, H + 2, Wd + 2, Cc))
            return (lambda: ctx.lib.me_op_nhwc32_to_16b(ctx.handle, p(S), p(o), B, H, Wd, Cc, relu)), {"dst16b": o}

        got = settle(run_both(ctx, build16b), masks={"dst16b": inner})["dst16b"]
        same(got[:, 1:-1, 1:-1], (u.clamp_min(0.0) if relu else u).to(T), zero_sign=not relu)


@pytest.mark.parametrize("dtype", DTYPES)
def test_concat_and_fov_add(dtype):
    """one pixel of 8 + 8 channels; fov_add at grid 8, batch 1, C 64 (the cls row of `lin` is skipped, the border keeps the fill)"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(64 * 4)  # one pixel
    a, b = LT.values((1, 8), 1).to(T), LT.values((1, 8), 2).to(T)

    def build(fs):
        A, Bt = fs.inp(a), fs.inp(b)
        o = fs.out(T, (1, 16))
        return (lambda: ctx.lib.me_op_concat_channels(ctx.handle, p(A), p(Bt), p(o), 1, 8, 8)), {"dst16": o}

    same(settle(run_both(ctx, build))["dst16"], R.concat_channels(a, b))
    grid, batch, Cc = 8, 1, 64
    P = grid * grid
    lin, low = LT.values((batch, P + 1, Cc), grid + Cc), LT.values((batch, P, Cc), grid + Cc + 1, scale=0.5)
    lin[lin.abs() > 3.0e4] = 1.0
    low[low.abs() > 3.0e4] = -1.0

    def build_f(fs):
        L_, W_ = fs.inp(lin), fs.inp(low)
        o = fs.out(T, (batch, grid + 2, grid + 2, Cc))
        return (lambda: ctx.lib.me_op_fov_add(ctx.handle, p(L_), p(W_), p(o), batch, grid, Cc, P + 1)), {"dst16b": o}

    inner = torch.zeros(batch, grid + 2, grid + 2, dtype=torch.bool)
    inner[:, 1:-1, 1:-1] = True
    got = settle(run_both(ctx, build_f), masks={"dst16b": inner})["dst16b"]
    same(got[:, 1:-1, 1:-1], R.fov_add(lin, low, grid).to(T))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fov_final(dtype):
    """(batch 1, k 1, C 8) at 5 degrees: eight products on 256 threads; bounds: test_gpu_layout.py test_fov_final"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(8 * 4)  # the k x k x C products
    batch, k, Cc, target = 1, 1, 8, 5.0
    n = k * k * Cc
    g = torch.Generator().manual_seed(n + int(target))
    base = torch.rand(n, generator=g) + 0.5
    x = (base[None, :] * (1.0 + 0.002 * torch.randn(batch, n, generator=g))).to(T)
    w0 = torch.randn(n, generator=g)
    bias = torch.tensor([0.25])
    w = (w0 * ((target - 0.25) / float(x[0].double() @ w0.double()))).float()

    def build(fs):
        X, Wt, b = fs.inp(x), fs.inp(w), fs.inp(bias)
        deg, fn = fs.out(F32, (batch,)), fs.out(F32, (batch,))
        return (lambda: ctx.lib.me_op_fov_final(ctx.handle, p(X), p(Wt), p(b), p(deg), p(fn), batch, k, Cc)), {"fov_deg": deg, "f_norm": fn}

    got = settle(run_both(ctx, build))
    prod = x.double() * w.double()
    ref = prod.sum(dim=1) + 0.25
    deg = got["fov_deg"].double().cpu()
    assert bool(((deg - ref).abs() <= n * 2.0 ** -24 * prod.abs().sum(dim=1)).all())
    half = 0.5 * deg * math.pi / 180.0
    want = torch.tan(half) / 0.5
    kappa = half * (1 + torch.tan(half) ** 2) / torch.tan(half)
    assert bool((((got["f_norm"].double().cpu() - want) / want).abs() <= 2.0 ** -24 * (4 + 4 * kappa)).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [4, 4100])
def test_casts(dtype, count):
    """one vector of four, and 4100 = 16 workgroups of 256 and one lane; exact"""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    tile(256 * 16)  # one vector per lane of a workgroup
    v = LT.values((count,), count)

    def build(fs):
        S = fs.inp(v)
        o = fs.out(T, (count,))
        return (lambda: ctx.lib.me_op_cast_to16(ctx.handle, p(S), p(o), count)), {"dst16": o}

    ctx.status_flags()
    same(settle(run_both(ctx, build))["dst16"], v.to(T))
    assert ctx.status_flags() == 0
    v16 = v.to(T)

    def build_back(fs):
        S = fs.inp(v16)
        o = fs.out(F32, (count,))
        return (lambda: ctx.lib.me_op_cast_to32(ctx.handle, p(S), p(o), count)), {"dst": o}

    same(settle(run_both(ctx, build_back))["dst"], v16.float())


# ---------------------------------------------------------------------------------------------------------------------
# byte-stream helpers: exact, as in their own tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n", [1, 257])
def test_exclusive_scan(form, n):
    """one count, and one more than a workgroup of the two-level scan; against numpy.cumsum in uint64 (test_gpu_scan.py)"""
    ctx = ctx_for("tiny", "f16")
    tile(1024 * 8)  # one element per thread of the one-workgroup scan
    counts = np.random.default_rng(1000 + n).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    base = (1 << 32) + 12345
    want = np.zeros(n + 1, np.uint64)
    np.cumsum(counts.astype(np.uint64), out=want[1:])

    def build(fs):
        c = fs.inp(torch.from_numpy(counts.view(np.int32).copy()))
        o = fs.out(torch.int64, (n + 1,))
        return (lambda: ctx.lib.me_op_exclusive_scan_u32(ctx.handle, p(c), n, base, form, p(o))), {"offsets": o}

    got = settle(run_both(ctx, build), raw=("offsets",))["offsets"].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want + np.uint64(base))


@pytest.mark.parametrize("colours", [0, 1])
def test_ply_pack(colours):
    """5 vertices, 3 faces, a 7-byte header in front of the records: the header's bytes keep the fill, and the records start off
    every alignment; against ply_cases.ply_body_fast (test_gpu_ply.py)"""
    import ply_cases as P
    ctx = ctx_for("tiny", "f16")
    tile(256 * 27)  # the records of one workgroup
    xyz, faces, rgb = P.random_mesh(5, 3, 9)
    header = 7
    body = 5 * (27 if colours else 24) + 3 * 13

    def build(fs):
        X, Fc = fs.inp(torch.from_numpy(xyz)), fs.inp(torch.from_numpy(faces))
        Cl = fs.inp(torch.from_numpy(rgb)) if colours else None
        o = fs.out(U8, (header + body,))
        return (lambda: ctx.lib.me_op_ply_pack(ctx.handle, p(X), p(Cl), 5, p(Fc), 3, header, p(o))), {"out": o}

    written = torch.ones(header + body, dtype=torch.bool)
    written[:header] = False
    got = settle(run_both(ctx, build), masks={"out": written}, raw=("out",))["out"].cpu().numpy().tobytes()
    assert got[header:] == P.ply_body_fast(xyz, faces, rgb if colours else None)


def test_format_f64():
    """three values into 344-byte slots: the bytes behind each number's length keep the fill; against the oracle's rust_display_f64
    (test_gpu_output.py)"""
    from oracle import output_oracle as OO
    ctx = ctx_for("tiny", "f16")
    tile(344)
    vals = np.array([0.1, -123456.789e-12, 1.7976931348623157e308], np.float64)
    stride = 344
    want = [OO.rust_display_f64(float(v)).encode() for v in vals]

    def build(fs):
        V = fs.inp(torch.from_numpy(vals))
        text, lens = fs.out(U8, (3, stride)), fs.out(torch.int32, (3,))
        return (lambda: ctx.lib.me_op_format_f64(ctx.handle, p(V), 3, p(text), stride, p(lens))), {"text": text, "lengths": lens}

    written = torch.zeros(3, stride, dtype=torch.bool)
    for i, w in enumerate(want):
        written[i, :len(w)] = True
    got = settle(run_both(ctx, build), masks={"text": written}, raw=("text", "lengths"))
    assert got["lengths"].cpu().tolist() == [len(w) for w in want]
    text = got["text"].cpu().numpy()
    for i, w in enumerate(want):
        assert text[i, :len(w)].tobytes() == w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,dims,dup", [(W.K_VEC_F32, (257,), 0), (W.K_MAT_16, (3, 5), 0), (W.K_CONV_16, (3, 5, 3, 3), 1),
                                           (W.K_CONVT_16, (5, 7, 2, 2), 0), (W.K_CONVK_F32, (1, 5, 3, 3), 0)])
def test_weight_pack(dtype, kind, dims, dup):
    """one tensor per kind from an f32 source, [W | W] on the convolution; exact against weight_pack_cases.py (its sources carry
    NaN and infinities on purpose: they must arrive as such)"""
    ctx = ctx_for("tiny", dtype)
    tile(64 * 64 * 4)  # one transposing tile
    src = W.source(dims, W.W_F32, seed=31)
    n = W.dst_elems(kind, dims, dup)
    dt = torch.int16 if W.dst_dtype(kind) == np.uint16 else torch.int32
    cdims = (C.c_int64 * len(dims))(*dims)

    def build(fs):
        S = fs.inp(torch.from_numpy(src.reshape(-1).copy()))
        o = fs.out(dt, (n,))
        return (lambda: ctx.lib.me_op_weight_pack(ctx.handle, kind, dup, cdims, len(dims), p(S), W.W_F32, p(o))), {"dst": o}

    got = settle(run_both(ctx, build), raw=("dst",))["dst"].cpu().numpy().view(W.dst_dtype(kind))
    W.check(got, kind, dims, dup, src, W.W_F32, dtype)


def test_png_unfilter():
    """the filtered stream of a 65-row picture in device memory, in bands of 2 rows and at the default; exact against the host
    restatement of test_gpu_png_decode.py"""
    import png_files as PF
    import test_gpu_png_decode as PD
    ctx = ctx_for("tiny", "f16")
    tile(64 * 4 * 1024)  # the row group of a workgroup
    stream, (w, h, depth, ctype, il) = PD._stream_of(dict(PF.FILES)["rows65"]())
    want = PD._unfiltered_reference(stream, (w, h, depth, ctype, il))
    for band_rows in (2, 0):

        def build(fs):
            S = fs.inp(torch.from_numpy(stream.copy()))
            o = fs.out(U8, (len(stream),))
            return (lambda: ctx.lib.me_op_png_unfilter(ctx.handle, p(S), len(stream), w, h, depth, ctype, il, band_rows, p(o))), {"out": o}

        got = settle(run_both(ctx, build), raw=("out",))["out"].cpu().numpy()
        assert np.array_equal(got, want), band_rows


def test_jpeg_entropy():
    """the coefficients of a 64 x 48 picture into device memory (the file itself is a host array by the entry's rule); exact
    against me_op_jpeg_coefficients_host (test_gpu_jpeg_entropy.py)"""
    import jpeg_files as J
    ctx = ctx_for("tiny", "f16")
    tile(65536 // 8)  # the longest subsequence
    data = J.plain(64, 48)
    import test_gpu_jpeg_entropy as JE
    want = JE.host_coefficients("64x48", data)

    def build(fs):
        o = fs.out(torch.int16, (want.size,))
        return (lambda: ctx.lib.me_op_jpeg_entropy(ctx.handle, data, len(data), 64, p(o), want.size)), {"coef": o}

    got = settle(run_both(ctx, build), raw=("coef",))["coef"].cpu().numpy()
    assert np.array_equal(got, np.asarray(want).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------
# the harness sees an overrun
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fences_report_an_overrun(dtype):
    """me_op_cast_to16 told to convert count = n + 4 elements on fences sized for n: it reads 16 bytes of the source's back guard
    and writes 8 bytes into the destination's, all inside the two allocations.  The source's guard is 0x00 (0.0, which converts
    to 0x0000) and the destination's 0xFF, so the eight bytes written differ from the fill: tampered() reports exactly those
    offsets, the front guard and the source fence stay clean, the payload is the cast of the n values."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    n = 260
    v = LT.values((n,), 5)
    src, dst = RZ.Fence(n * 4, 0x00), RZ.Fence(n * 2, 0xFF)
    src.view(F32, (n,)).copy_(v)
    src.snapshot()
    assert (n + 4) * 4 <= n * 4 + RZ.GUARD and (n + 4) * 2 <= n * 2 + RZ.GUARD          # the access stays inside the allocations
    torch.cuda.synchronize()
    rc = ctx.lib.me_op_cast_to16(ctx.handle, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n + 4)
    ctx.synchronize()
    ctx.status_flags()
    assert rc == 0
    assert dst.tampered() == list(range(2 * n, 2 * n + 8))
    assert bool((dst.back[:8] == 0).all()) and bool((dst.back[8:] == 0xFF).all()) and bool((dst.front == 0xFF).all())
    assert src.tampered() == [] and src.unchanged()
    same(dst.view(T, (n,)), v.to(T))


def test_every_entry_was_called_between_fences(request):
    """The last test of the file: every name of COVERED was really asked of the library inside run_both by the tests above -- a
    listed entry whose call was dropped from its test's body fails here.  Only a run of the whole file can say so: under a -k
    expression or a node id nothing is held."""
    if request.config.getoption("keyword") or any("::" in a for a in request.config.args):
        return
    missing = sorted(set(COVERED) - CALLED)
    assert not missing, missing
