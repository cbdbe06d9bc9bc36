"""Kernel-level tests (-m gpu) of the layout / element-wise kernels of csrc/elementwise.hip and of the patch-embed
epilogue, each through its own entry point (include/matrix_eyes_hip_ops.h).  All but bilinear, the patch embed and
the FOV dot product are data movement plus at most one rounding and are held BIT FOR BIT to tests/layout_refs.py
(itself tied to the oracle by test_layout_refs_cpu.py); outputs are pre-filled with a sentinel so that an element the
kernel must not write (borders, cls rows, guard rows behind the buffer) shows when it is overwritten."""
import math

import pytest
import torch

import layout_refs as R
from oracle import depth_pro_oracle as O
from util import TORCH16, ctx_for, loaded_ctx, max_abs_rel, ptr

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SENT = -7.5                    # exact in f16, bf16 and f32; no kernel under test produces it from the inputs below
GUARD = 4096                   # sentinel elements behind every output
TRIP = 16384 * 256             # work items of one trip of a grid-stride loop (elementwise.hip grid_for)


def call(ctx, fn, *args):
    """One launch on the context's stream, fenced on both sides: the buffers were filled on torch's stream."""
    torch.cuda.synchronize()
    ctx._check(fn(ctx.handle, *args))
    ctx.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, want, zero_sign=True):
    """Raw equality of two tensors of one type (zero_sign=False: +0 and -0 are one value -- max(-0, +0) is either)."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    eq = bits(got) == bits(want)
    if not zero_sign:
        eq |= (got == 0) & (want == 0)
    if not bool(eq.all()):
        bad = (~eq).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{int((~eq).sum())} of {eq.numel()} elements differ; first at {i}: got {got[i].item()!r}, "
                             f"want {want[i].item()!r}")


def out_buf(numel, dt):
    """numel + GUARD elements of the sentinel; returns (whole buffer, guard view)."""
    buf = torch.full((numel + GUARD,), SENT, dtype=dt, device="cuda")
    return buf, buf[numel:]


def guard_ok(guard):
    assert bool((guard == SENT).all()), "the kernel wrote behind its output"


def values(shape, seed, scale=1.0):
    """Seeded f32 noise with the awkward values planted: +-0, f16 subnormals, f16 rounding ties (to even, both ways),
    the f16 maximum (nothing beyond it: these are the CLEAN inputs, which must not raise the overflow status)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g) * scale
    sp = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15 + 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24,
                       1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2049.0, 2051.0, 65504.0, -65504.0,
                       1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.1, 1e-9, 1.0 / 3.0])
    flat = v.reshape(-1)
    idx = torch.randint(0, flat.numel(), (min(flat.numel() // 2, 40 * sp.numel()),), generator=g)
    flat[idx] = sp.repeat(40)[:idx.numel()]
    return v


# ---------------------------------------------------------------------------------------------------------------
# patchify, patchify_windows, cls_rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,grid,batch", [("f16", 8, 1), ("f16", 8, 3), ("f16", 24, 3), ("f16", 32, 1), ("f16", 40, 1),
                                              ("f16", 64, 1), ("bf16", 8, 3), ("bf16", 24, 1)])
def test_patchify(dtype, grid, batch):
    """patchify_kernel against layout_refs.patchify, bit for bit (a copy: one instantiation serves both types, so the
    large grids run on one).  (24, 3) and (64, 1) have more than one trip of the grid-stride loop."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    wp, P = 16 * grid, grid * grid
    xs = [values((batch, 3, s * wp, s * wp), grid * 10 + s).to(T) for s in (4, 2, 1)]
    want = R.patchify(xs[0], xs[1], xs[2], grid)
    dev = [x.cuda() for x in xs]
    n = batch * 35 * P * 768
    if (grid, batch) in ((24, 3), (64, 1)):
        assert batch * 35 * P * 96 > TRIP
    buf, guard = out_buf(n, T)
    call(ctx, ctx.lib.me_op_patchify, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(buf), batch, grid)
    same_bits(buf[:n].reshape(-1, 768), want)
    guard_ok(guard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,windows", [(8, 1), (8, 35), (24, 3), (40, 35), (64, 1)])
def test_patchify_windows(dtype, grid, windows):
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    P = grid * grid
    xs = values((windows, 3, 16 * grid, 16 * grid), grid + windows).to(T)
    want = R.patchify_windows(xs, grid)
    if (grid, windows) == (40, 35):
        assert windows * P * 96 > TRIP
    n = windows * P * 768
    buf, guard = out_buf(n, T)
    xd = xs.cuda()
    call(ctx, ctx.lib.me_op_patchify_windows, ptr(xd), ptr(buf), windows, grid)
    same_bits(buf[:n].reshape(-1, 768), want)
    guard_ok(guard)


@pytest.mark.parametrize("windows,tpw,dim", [(1, 65, 128), (35, 577, 64), (105, 65, 1024), (4200, 2, 1024)])
def test_cls_rows(windows, tpw, dim):
    """Row 0 of every window = cls + pos[0] (one f32 addition); every other row keeps the sentinel.  The last case has
    more than one trip of the grid-stride loop."""
    ctx = ctx_for("tiny", "f16")
    cls, pos = values((dim,), 1), values((tpw, dim), 2)
    n = windows * tpw * dim
    if windows == 4200:
        assert windows * dim > TRIP
    buf, guard = out_buf(n, torch.float32)
    cd, pd = cls.cuda(), pos.cuda()
    call(ctx, ctx.lib.me_op_cls_rows, ptr(buf), ptr(cd), ptr(pd), windows, tpw, dim)
    want = R.cls_rows(torch.full((windows, tpw, dim), SENT), cls, pos)
    same_bits(buf[:n].reshape(windows, tpw, dim), want)
    guard_ok(guard)


# ---------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------
def _merge_geometries(grid):
    """(wpi, win0, steps, padding) as pipeline.hip passes them: the 25 windows of level 0, the 9 of level 1, the one of
    level 2, and the image encoder's single window."""
    return [(35, 0, 5, grid // 8), (35, 25, 3, grid // 4), (35, 34, 1, 0), (1, 0, 1, 0)]


def _merge_case(ctx, dtype, grid, batch, dim, geom, source, split, seed):
    T = TORCH16[dtype]
    wpi, win0, steps, padding = geom
    P1 = grid * grid + 1
    tok = values((batch * wpi, P1, dim), seed)
    if source == 16:
        tok = tok.to(T)
    ref = R.merge(tok, batch, wpi, win0, steps, padding, grid)
    want = R.split_pixels(ref, T) if split else ref.to(T)
    side = ref.shape[1]
    n = want.numel()
    buf, guard = out_buf(n, T)
    td = tok.cuda()
    ctx.status_flags()
    call(ctx, ctx.lib.me_op_merge, ptr(td) if source == 32 else None, ptr(td) if source == 16 else None, ptr(buf),
         batch, wpi, win0, steps, padding, grid, dim, split)
    same_bits(buf[:n].reshape(want.shape), want)
    guard_ok(guard)
    assert ctx.status_flags() == 0          # the inputs reach 65504 and no further
    return batch * side * side * (dim // 8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,batch,dim", [(8, 1, 64), (8, 3, 64), (24, 3, 32), (32, 1, 40), (40, 3, 16), (64, 1, 8)])
def test_merge(dtype, grid, batch, dim):
    """merge_kernel (reshape_feature + merge as one row gather) against layout_refs.merge, bit for bit: the three
    window geometries of the patch encoder and the image encoder's single window; f32 source rounded once, f32 source
    split into [hi | lo], 16-bit source copied."""
    ctx = ctx_for("tiny", dtype)
    for gi, geom in enumerate(_merge_geometries(grid)):
        for source, split in ((32, 0), (32, 1), (16, 0)):
            _merge_case(ctx, dtype, grid, batch, dim, geom, source, split, 1000 * grid + 10 * gi + source + split)


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_second_trip(dtype):
    """More than 16384 x 256 work items: the second trip of the grid-stride loop, split f32 source and 16-bit source."""
    ctx = ctx_for("tiny", dtype)
    for source, split in ((32, 1), (16, 0)):
        items = _merge_case(ctx, dtype, 32, 3, 768, (35, 0, 5, 4), source, split, 77 + source)
        assert items > TRIP


# ---------------------------------------------------------------------------------------------------------------
# the four layout changes, concat, fov_add
# ---------------------------------------------------------------------------------------------------------------
MAPS = [(1, 37, 5, 7), (3, 100, 9, 13), (2, 64, 24, 24), (1, 8, 33, 31)]       # (B, C, H, W): H W and C off the 32 x 32 tiles


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MAPS)
def test_nchw32_to_nhwc(dtype, shape):
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    B, C, H, W = shape
    x = values(shape, sum(shape))
    xd = x.cuda()
    nhwc = R.nchw_to_nhwc(x)
    ctx.status_flags()
    for border in (0, 1):
        for relu16 in (0, 1):
            for split in (0, 1):
                for with32 in (0, 1):
                    a = nhwc.clamp_min(0.0) if relu16 else nhwc
                    w16 = R.split_pixels(a, T) if split else a.to(T)
                    Cw = w16.shape[-1]
                    canvas = torch.full((B, H + 2 * border, W + 2 * border, Cw), SENT, dtype=T)
                    want16 = R.into_border(canvas, w16) if border else w16
                    b16, g16 = out_buf(want16.numel(), T)
                    b32, g32 = out_buf(nhwc.numel(), torch.float32)
                    call(ctx, ctx.lib.me_op_nchw32_to_nhwc, ptr(xd), ptr(b32) if with32 else None, ptr(b16), B, H, W, C,
                         border, relu16, split)
                    tag = (border, relu16, split, with32)
                    try:
                        same_bits(b16[:want16.numel()].reshape(want16.shape), want16, zero_sign=not relu16)
                        if with32:
                            same_bits(b32[:nhwc.numel()].reshape(nhwc.shape), nhwc)       # the f32 copy is never clamped
                        else:
                            assert bool((b32 == SENT).all())
                    except AssertionError as e:
                        raise AssertionError(f"{tag}: {e}") from None
                    guard_ok(g16), guard_ok(g32)
    # f32 copy alone
    b32, g32 = out_buf(nhwc.numel(), torch.float32)
    call(ctx, ctx.lib.me_op_nchw32_to_nhwc, ptr(xd), ptr(b32), None, B, H, W, C, 0, 0, 0)
    same_bits(b32[:nhwc.numel()].reshape(nhwc.shape), nhwc)
    guard_ok(g32)
    assert ctx.status_flags() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MAPS)
def test_nhwc_to_nchw(dtype, shape):
    """nhwc_to_nchw_kernel, both source types: 16-bit (border 0 / 1, split 0 / 1: value = hi + lo, one f32 addition)
    and f32."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    B, C, H, W = shape
    v = R.nchw_to_nhwc(values(shape, sum(shape) + 1))
    n = B * C * H * W
    for border in (0, 1):
        for split in (0, 1):
            src = R.split_pixels(v, T) if split else v.to(T)
            want = R.nhwc_to_nchw((src[..., :C].float() + src[..., C:].float()) if split else src.float())
            if border:   # the border holds the sentinel: a kernel that read it would carry it into the result
                src = R.into_border(torch.full((B, H + 2, W + 2, src.shape[-1]), SENT, dtype=T), src)
            sd = src.cuda()
            buf, guard = out_buf(n, torch.float32)
            call(ctx, ctx.lib.me_op_nhwc16_to_nchw32, ptr(sd), ptr(buf), B, H, W, C, border, split)
            try:
                same_bits(buf[:n].reshape(want.shape), want)
            except AssertionError as e:
                raise AssertionError(f"border {border} split {split}: {e}") from None
            guard_ok(guard)
    vd = v.cuda()
    buf, guard = out_buf(n, torch.float32)
    call(ctx, ctx.lib.me_op_nhwc32_to_nchw32, ptr(vd), ptr(buf), B, H, W, C)
    same_bits(buf[:n].reshape(B, C, H, W), R.nhwc_to_nchw(v))
    guard_ok(guard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 5, 7, 12), (3, 9, 13, 100), (2, 24, 24, 64), (3, 128, 128, 384)])
def test_nhwc32_to_16b(dtype, shape):
    """f32 NHWC -> the interior of a bordered 16-bit map, with and without ReLU; the border keeps the sentinel.  The last
    case has more than one trip of the grid-stride loop."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    B, H, W, C = shape
    if shape[1] == 128:
        assert B * H * W * (C // 4) > TRIP
    v = values(shape, sum(shape) + 2)
    vd = v.cuda()
    ctx.status_flags()
    for relu in (0, 1):
        want = R.into_border(torch.full((B, H + 2, W + 2, C), SENT, dtype=T), (v.clamp_min(0.0) if relu else v).to(T))
        buf, guard = out_buf(want.numel(), T)
        call(ctx, ctx.lib.me_op_nhwc32_to_16b, ptr(vd), ptr(buf), B, H, W, C, relu)
        same_bits(buf[:want.numel()].reshape(want.shape), want, zero_sign=not relu)
        guard_ok(guard)
    assert ctx.status_flags() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pixels,Ca,Cb", [(1, 8, 8), (77, 24, 104), (576, 256, 256), (3 * 96 * 96, 1024, 256)])
def test_concat_channels(dtype, pixels, Ca, Cb):
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    if pixels > 1000:
        assert pixels * (Ca + Cb) // 8 > TRIP
    a, b = values((pixels, Ca), pixels).to(T), values((pixels, Cb), pixels + 1).to(T)
    want = R.concat_channels(a, b)
    buf, guard = out_buf(want.numel(), T)
    ad, bd = a.cuda(), b.cuda()
    call(ctx, ctx.lib.me_op_concat_channels, ptr(ad), ptr(bd), ptr(buf), pixels, Ca, Cb)
    same_bits(buf[:want.numel()].reshape(want.shape), want)
    guard_ok(guard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,batch,C,extra", [(8, 1, 64, 0), (8, 3, 20, 5), (24, 3, 128, 0), (32, 1, 36, 2), (40, 1, 8, 0),
                                                (64, 3, 384, 0)])
def test_fov_add(dtype, grid, batch, C, extra):
    """fov_add_kernel: T(lin[b][1 + p][c] + low[b][p][c]) into the interior of the bordered map -- one rounding of one
    f32 sum, so bit for bit.  tpw = g * g + 1 + extra rows per window in lin (the cls row first); the last case has more
    than one trip of the grid-stride loop."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    P = grid * grid
    tpw = P + 1 + extra
    if grid == 64:
        assert batch * P * C > TRIP
    lin, low = values((batch, tpw, C), grid + C), values((batch, P, C), grid + C + 1, scale=0.5)
    lin[lin.abs() > 3.0e4] = 1.0        # (clean inputs: no SUM may leave the f16 range)
    low[low.abs() > 3.0e4] = -1.0
    # ties of the SUM: 1 + 2^-11 rounds to even (down), 1 + 3 * 2^-11 up; a sum of two halves of the f16 maximum
    lin[0, 1, :4] = torch.tensor([1.0, 1.0, 32752.0, -0.0])
    low[0, 0, :4] = torch.tensor([2.0 ** -11, 3 * 2.0 ** -11, 32752.0, 0.0])
    want = R.into_border(torch.full((batch, grid + 2, grid + 2, C), SENT, dtype=T),
                         R.fov_add(lin[:, :P + 1], low, grid).to(T))
    buf, guard = out_buf(want.numel(), T)
    ld, wd = lin.cuda(), low.cuda()
    ctx.status_flags()
    call(ctx, ctx.lib.me_op_fov_add, ptr(ld), ptr(wd), ptr(buf), batch, grid, C, tpw)
    same_bits(buf[:want.numel()].reshape(want.shape), want)
    guard_ok(guard)
    assert ctx.status_flags() == 0


# ---------------------------------------------------------------------------------------------------------------
# bilinear
# ---------------------------------------------------------------------------------------------------------------
def _half_ulp(x, T):
    """Half the spacing of T's grid at magnitude x (f64 tensor), with the subnormal floor: one rounding."""
    fi = torch.finfo(T)
    mant = {torch.float16: 10, torch.bfloat16: 7}[T]
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(fi.smallest_normal))) - mant - 1)


def _neighbourhood(src, out_size, align):
    """Per output element: spread R and largest magnitude A of the source texels of the reference's cell and of its
    neighbours one texel out (f64 [planes][out][out])."""
    planes, n, _ = src.shape
    o = torch.arange(out_size, dtype=torch.float64)
    pos = o * ((n - 1) / max(out_size - 1, 1)) if align else ((o + 0.5) * (n / out_size) - 0.5).clamp_min(0.0)
    i0 = pos.floor().long().clamp(max=n - 1)
    hi = torch.full((planes, out_size, out_size), -math.inf, dtype=torch.float64)
    lo = torch.full_like(hi, math.inf)
    for dy in (-1, 0, 1, 2):
        ys = (i0 + dy).clamp(0, n - 1)
        for dx in (-1, 0, 1, 2):
            xs = (i0 + dx).clamp(0, n - 1)
            t = src[:, ys][:, :, xs]
            hi, lo = torch.maximum(hi, t), torch.minimum(lo, t)
    return hi - lo, torch.maximum(hi.abs(), lo.abs())


def _bilinear_check(ctx, dtype, src, out_size, align):
    """Bounds, per element, against O.interpolate_bilinear in fp64.
    align_corners = 0 at ratios 2 and 4: (o + 0.5) * ratio - 0.5 and the weights (multiples of 1/8) are exact in f32, so
    the f32 value differs from the reference by the roundings of four weighted texels and three additions of a convex
    combination, at most 4 * 2^-24 * max|texel|, and is then rounded once to 16 bit.
    align_corners = 1: the kernel forms ratio = f32((in - 1) / (out - 1)) and ratio * y in f32: two roundings of a
    position below in - 1, so the position is off by at most delta = 2^-23 * (in - 1) on each axis.  A bilinear surface
    changes by at most R per texel along an axis, R the spread of the texels around the position (the cell's four; taken
    here over the cell and its neighbours one texel out, because a position within delta of a cell boundary may be
    evaluated in the neighbouring cell -- the surface is continuous across it, its slope is the neighbour's): 2 * delta *
    R.  The weights 1 - w, the four products and three additions: at most 8 * 2^-24 * A, A the largest magnitude
    among those texels.  One rounding to 16 bit: eps16 * |ref| (half an ulp at the value rounded)."""
    T = TORCH16[dtype]
    planes, n, _ = src.shape
    sd = src.cuda()
    cnt = planes * out_size * out_size
    buf, guard = out_buf(cnt, T)
    ctx.status_flags()
    call(ctx, ctx.lib.me_op_bilinear, ptr(sd), ptr(buf), planes, n, out_size, align)
    guard_ok(guard)
    assert ctx.status_flags() == 0
    got = buf[:cnt].reshape(planes, out_size, out_size).double().cpu()
    ref = O.interpolate_bilinear(src.double()[None], out_size, out_size, bool(align))[0]
    Rn, A = _neighbourhood(src.double(), out_size, align)
    if align:
        delta = 2.0 ** -23 * (n - 1)
        slack = 2 * delta * Rn + 8 * 2.0 ** -24 * A
    else:
        assert n in (2 * out_size, 4 * out_size)
        slack = torch.full_like(ref, 4 * 2.0 ** -24 * float(src.abs().max()))
    bound = _half_ulp(ref.abs() + slack, T) + slack
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"bilinear {dtype} {planes}x{n}->{out_size} align {align}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    return got, ref, bound


def _ramp(planes, n):
    y, x = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    return torch.stack([(0.25 * (p + 1)) * y - 0.125 * x + (p - 1.0) for p in range(planes)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,out_size,planes,align", [
    (1536, 768, 9, 1), (1536, 384, 3, 1), (128, 64, 3, 1), (128, 32, 2, 1), (37, 11, 2, 1), (7, 13, 1, 1), (50, 50, 1, 1), (33, 1, 2, 1),
    (2, 5, 1, 1), (1536, 768, 9, 0), (1536, 384, 3, 0), (128, 64, 3, 0), (128, 32, 2, 0), (20, 10, 1, 0), (12, 3, 2, 0)])
def test_bilinear(dtype, n, out_size, planes, align):
    """bilinear_kernel on noise and on a ramp (whose resampling is known in closed form); the pyramid's own 1536 -> 768
    and -> 384 (nine planes: more than one trip of the grid-stride loop), odd sizes, out_size = 1."""
    ctx = ctx_for("tiny", dtype)
    if planes == 9:
        assert planes * out_size * out_size > TRIP
    noise = values((planes, n, n), n + out_size)
    noise[noise.abs() > 100] = 1.0               # (the planted f16 maximum: kept for the overflow test below)
    _bilinear_check(ctx, dtype, noise, out_size, align)
    ramp = _ramp(planes, n)
    got, ref, bound = _bilinear_check(ctx, dtype, ramp, out_size, align)
    # closed form: a ramp a y + b x + c sampled at (sy, sx) is a sy + b sx + c
    o = torch.arange(out_size, dtype=torch.float64)
    s = o * ((n - 1) / max(out_size - 1, 1)) if align else ((o + 0.5) * (n / out_size) - 0.5).clamp_min(0.0)
    s = s.clamp(max=n - 1)
    closed = torch.stack([(0.25 * (p + 1)) * s[:, None] - 0.125 * s[None, :] + (p - 1.0) for p in range(planes)])
    assert float((ref - closed).abs().max()) < 1e-9 * n
    assert bool(((got - closed).abs() <= bound + 1e-9 * n).all())
    if align and out_size > 1:
        # the `out - 1` denominator: the last output row and column are the last input row and column
        last_row = O.interpolate_bilinear(ramp.double()[None, :, -1:, :].expand(1, planes, 2, n), 2, out_size, True)[0, :, 0]
        assert float((ref[:, -1, :] - last_row).abs().max()) < 1e-9 * n
        assert bool(((got[:, -1, :] - last_row).abs() <= bound[:, -1, :] + 1e-9 * n).all())
        assert bool(((got[:, :, -1] - ref[:, :, -1]).abs() <= bound[:, :, -1]).all())
        assert bool(((got[:, -1, -1] - ramp.double()[:, -1, -1]).abs() <= bound[:, -1, -1]).all())


# ---------------------------------------------------------------------------------------------------------------
# patch embed, fov_final
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("windows,P,C,cfg", [(1, 64, 128, -1), (35, 576, 256, -1), (105, 64, 1024, -1), (35, 64, 132, 0), (3, 65, 64, 1)])
def test_patch_embed(dtype, windows, P, C, cfg):
    """EPI_PATCH_EMBED: patches . W^T + bias + pos[1 + p] into rows 1 .. P of every window's P + 1 token rows, in fp64 on
    the same 16-bit operands; max_abs_rel < 1e-4, the project's bound for f32 accumulation over K up to 4096.  The cls
    rows and the guard keep the sentinel."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    g = torch.Generator().manual_seed(windows + P + C)
    patches = torch.randn(windows * P, 768, generator=g).to(T).cuda()
    w = (torch.randn(C, 768, generator=g) / math.sqrt(768)).to(T).cuda()
    bias, pos = torch.randn(C, generator=g).cuda(), torch.randn(P + 1, C, generator=g).cuda()
    n = windows * (P + 1) * C
    buf, guard = out_buf(n, torch.float32)
    call(ctx, ctx.lib.me_op_patch_embed, ptr(patches), windows, P, C, ptr(w), ptr(bias), ptr(pos), ptr(buf), cfg)
    tok = buf[:n].reshape(windows, P + 1, C)
    ref = R.patch_embed_tokens(patches, w, bias, pos, torch.zeros(C, device="cuda"), P)
    err = max_abs_rel(tok[:, 1:], ref[:, 1:])
    print(f"patch embed {dtype} {windows}x{P}x{C} cfg {cfg}: max_abs_rel {err:.2e}")
    assert err < 1e-4
    assert bool((tok[:, 0] == SENT).all()), "a cls row was written"
    guard_ok(guard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch,k,C", [(1, 6, 32), (8, 3, 40), (8, 2, 100), (1, 1, 8)])
@pytest.mark.parametrize("target", [5.0, 60.0, 120.0, 170.0])
def test_fov_final(dtype, batch, k, C, target):
    """fov_deg against the fp64 dot product within the f32 summation bound n * 2^-24 * sum|x_i w_i|; f_norm against fp64
    tan(0.5 * deg * pi / 180) / 0.5 of the kernel's OWN deg, relative 2^-24 * (4 + 4 kappa) with kappa = x (1 + tan^2 x) /
    tan x the condition number of tan at the half angle x (the f32 argument carries about three roundings, tanf a few
    ulp).  n = k * k * C is not a multiple of the 256 threads."""
    ctx, T = ctx_for("tiny", dtype), TORCH16[dtype]
    n = k * k * C
    assert n % 256 != 0
    g = torch.Generator().manual_seed(n + int(target))
    base = torch.rand(n, generator=g) + 0.5
    x = (base[None, :] * (1.0 + 0.002 * torch.randn(batch, n, generator=g))).to(T)
    w0 = torch.randn(n, generator=g)
    bias = torch.tensor([0.25])
    w = (w0 * ((target - 0.25) / float(x[0].double() @ w0.double()))).float()
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    deg = torch.full((batch + 8,), SENT, device="cuda")
    fn = torch.full((batch + 8,), SENT, device="cuda")
    call(ctx, ctx.lib.me_op_fov_final, ptr(xd), ptr(wd), ptr(bd), ptr(deg), ptr(fn), batch, k, C)
    assert bool((deg[batch:] == SENT).all()) and bool((fn[batch:] == SENT).all())
    prod = x.double() * w.double()
    ref = prod.sum(dim=1) + 0.25
    got = deg[:batch].double().cpu()
    assert abs(float(ref[0]) - target) < 0.1
    bound = n * 2.0 ** -24 * prod.abs().sum(dim=1)
    assert bool(((got - ref).abs() <= bound).all()), (got, ref, bound)
    half = 0.5 * got * math.pi / 180.0
    want = torch.tan(half) / 0.5
    kappa = half * (1 + torch.tan(half) ** 2) / torch.tan(half)
    rel = ((fn[:batch].double().cpu() - want) / want).abs()
    print(f"fov_final {dtype} n {n} target {target}: deg err / bound {float(((got - ref).abs() / bound).max()):.3f}, "
          f"f_norm rel / bound {float((rel / (2.0 ** -24 * (4 + 4 * kappa))).max()):.3f}")
    assert bool((rel <= 2.0 ** -24 * (4 + 4 * kappa)).all()), (rel, kappa)
    # fov_deg == NULL: f_norm all the same
    fn2 = torch.full((batch,), SENT, device="cuda")
    call(ctx, ctx.lib.me_op_fov_final, ptr(xd), ptr(wd), ptr(bd), None, ptr(fn2), batch, k, C)
    assert torch.equal(fn2, fn[:batch])


# ---------------------------------------------------------------------------------------------------------------
# the overflow status (matrix_eyes_hip.h: every kernel that writes 16-bit operands raises ME_STATUS_OVERFLOW_16BIT)
# ---------------------------------------------------------------------------------------------------------------
def _overflow_launches(ctx, T, plant):
    """name -> launch, for every element-wise kernel that rounds f32 values to 16-bit operands; plant: the inputs hold
    one magnitude that does not fit f16 (7e4; for fov_add two addends of 4e4 and 3e4, each of which fits)."""
    big = 7.0e4 if plant else 1.0
    lib = ctx.lib
    keep = []

    def dev(t):
        keep.append(t.cuda())
        return keep[-1]

    def out(nel):
        keep.append(torch.zeros(nel, dtype=T, device="cuda"))
        torch.cuda.synchronize()        # (filled on torch's stream; the launch is on the context's)
        return keep[-1]

    def planted(shape, seed, at):
        v = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
        v[at] = -big
        return v

    B, C, H, W, g = 2, 40, 9, 11, 8
    P = g * g
    lin, low = planted((B, P + 1, 16), 1, (1, 5, 3)), torch.randn(B, P, 16, generator=torch.Generator().manual_seed(2))
    if plant:
        lin[1, 5, 3], low[1, 4, 3] = 4.0e4, 3.0e4
    tok = dev(planted((35, P + 1, 16), 3, (12, 1 + 3 * g + 4, 9)))      # window (2, 2) of the 5 x 5, token (3, 4): inside its crop
    nchw = dev(planted((B, C, H, W), 4, (1, 39, 8, 10)))
    nhwc = dev(planted((B, H, W, C), 5, (1, 8, 10, 39)))
    img = dev(planted((3, 64, 64), 6, (2, 63, 63)))
    flat = dev(planted((4096,), 7, (4095,)))
    lin_d, low_d = dev(lin), dev(low)
    return {
        "cast_to16": lambda: lib.me_op_cast_to16(ctx.handle, ptr(flat), ptr(out(4096)), 4096),
        "bilinear": lambda: lib.me_op_bilinear(ctx.handle, ptr(img), ptr(out(3 * 64 * 64)), 3, 64, 64, 1),
        "bilinear_half": lambda: lib.me_op_bilinear(ctx.handle, ptr(img), ptr(out(3 * 32 * 32)), 3, 64, 32, 1),
        "merge": lambda: lib.me_op_merge(ctx.handle, ptr(tok), None, ptr(out(96 * 96 * 16)), 1, 35, 0, 5, 1, g, 16, 0),
        "merge_split": lambda: lib.me_op_merge(ctx.handle, ptr(tok), None, ptr(out(96 * 96 * 32)), 1, 35, 0, 5, 1, g, 16, 1),
        "nchw32_to_nhwc": lambda: lib.me_op_nchw32_to_nhwc(ctx.handle, ptr(nchw), None, ptr(out(B * H * W * C)), B, H, W, C, 0, 0, 0),
        "nchw32_to_nhwc_split": lambda: lib.me_op_nchw32_to_nhwc(ctx.handle, ptr(nchw), None, ptr(out(B * (H + 2) * (W + 2) * 2 * C)),
                                                                B, H, W, C, 1, 0, 1),
        "nhwc32_to_16b": lambda: lib.me_op_nhwc32_to_16b(ctx.handle, ptr(nhwc), ptr(out(B * (H + 2) * (W + 2) * C)), B, H, W, C, 0),
        "fov_add": lambda: lib.me_op_fov_add(ctx.handle, ptr(lin_d), ptr(low_d), ptr(out(B * (g + 2) * (g + 2) * 16)), B, g, 16, P + 1),
    }, keep


@pytest.mark.parametrize("name", ["cast_to16", "bilinear", "bilinear_half", "merge", "merge_split", "nchw32_to_nhwc",
                                  "nchw32_to_nhwc_split", "nhwc32_to_16b", "fov_add"])
def test_overflow_status(name):
    """One magnitude past 65504 among the values a kernel rounds to f16 raises ME_STATUS_OVERFLOW_16BIT (read and
    cleared by me_status_flags); the same launch on a bf16 context raises nothing, and clean inputs raise nothing.
    bilinear with align_corners samples its last texel with weight one at out = in; at out = in / 2 the planted
    corner is still the last output's only texel (the `out - 1` denominator)."""
    f, b = ctx_for("tiny", "f16"), ctx_for("tiny", "bf16")
    f.status_flags(), b.status_flags()
    for ctx, T, plant, want in ((f, torch.float16, False, 0), (f, torch.float16, True, 1), (b, torch.bfloat16, True, 0),
                                (f, torch.float16, False, 0)):
        launches, keep = _overflow_launches(ctx, T, plant)
        ctx._check(launches[name]())
        ctx.synchronize()
        flags = ctx.status_flags()
        assert flags == want, f"{name}: status {flags}, expected {want} (f16 {T == torch.float16}, planted {plant})"
        assert ctx.status_flags() == 0
        del keep


def test_fov_forward_reports_an_overflowing_pixel():
    """me_fov_forward resamples the image itself (no cast of the full image in front of it, as the encoder has): a pixel
    past the f16 range must raise the status there."""
    import numpy as np
    import matrix_eyes_amd as m
    cfg = m.ModelConfig.tiny()
    S, g = cfg.img_size, cfg.grid
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 3, S, S)).astype(np.float32)
    low = rng.standard_normal((1, cfg.dec_dim, 2 * g, 2 * g)).astype(np.float32)
    ctx = loaded_ctx("tiny", "f16")
    ctx.status_flags()
    fov = ctx.fov_forward(x, low)
    assert np.isfinite(fov).all() and ctx.status_flags() == 0
    x[0, 1, :8, :8] = 7.0e4                      # whatever align_corners is, the first output pixel lies inside this block
    ctx.fov_forward(x, low)
    assert ctx.status_flags() == 1 and ctx.status_flags() == 0
    bctx = loaded_ctx("tiny", "bf16")
    bctx.status_flags()
    bctx.fov_forward(x, low)
    assert bctx.status_flags() == 0


# ---------------------------------------------------------------------------------------------------------------
# argument errors: rejected on the host, before any launch
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable():
    ctx = ctx_for("tiny", "f16")
    lib, h = ctx.lib, ctx.handle
    a = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    b = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    c = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    BAD_ARG, BAD_SHAPE = 1, 2
    cases = [
        (BAD_SHAPE, lambda: lib.me_op_merge(h, ptr(a), None, ptr(b), 1, 1, 0, 1, 0, 8, 12, 0)),            # dim % 8
        (BAD_SHAPE, lambda: lib.me_op_merge(h, ptr(a), None, ptr(b), 1, 1, 0, 1, 0, 12, 8, 0)),            # grid
        (BAD_SHAPE, lambda: lib.me_op_merge(h, ptr(a), None, ptr(b), 1, 35, 30, 3, 2, 8, 8, 0)),           # windows past wpi
        (BAD_ARG, lambda: lib.me_op_merge(h, ptr(a), ptr(c), ptr(b), 1, 1, 0, 1, 0, 8, 8, 0)),             # two sources
        (BAD_ARG, lambda: lib.me_op_merge(h, None, ptr(c), ptr(b), 1, 1, 0, 1, 0, 8, 8, 1)),               # split needs f32
        (BAD_ARG, lambda: lib.me_op_merge(h, ptr(a), None, None, 1, 1, 0, 1, 0, 8, 8, 0)),
        (BAD_SHAPE, lambda: lib.me_op_concat_channels(h, ptr(b), ptr(c), ptr(b), 4, 12, 8)),
        (BAD_SHAPE, lambda: lib.me_op_concat_channels(h, ptr(b), ptr(c), ptr(b), 0, 8, 8)),
        (BAD_SHAPE, lambda: lib.me_op_nhwc32_to_16b(h, ptr(a), ptr(b), 1, 4, 4, 6, 0)),                    # C % 4
        (BAD_SHAPE, lambda: lib.me_op_nhwc32_to_16b(h, ptr(a), ptr(b), 0, 4, 4, 8, 0)),
        (BAD_SHAPE, lambda: lib.me_op_bilinear(h, ptr(a), ptr(b), 1, 8, 0, 1)),
        (BAD_ARG, lambda: lib.me_op_bilinear(h, None, ptr(b), 1, 8, 4, 1)),
        (BAD_SHAPE, lambda: lib.me_op_patchify(h, ptr(b), ptr(b), ptr(b), ptr(c), 1, 0)),
        (BAD_SHAPE, lambda: lib.me_op_patchify_windows(h, ptr(b), ptr(c), 1, 20)),
        (BAD_SHAPE, lambda: lib.me_op_patchify_windows(h, ptr(b), ptr(c), 0, 8)),
        (BAD_SHAPE, lambda: lib.me_op_cls_rows(h, ptr(a), ptr(a), ptr(a), 1, 0, 8)),
        (BAD_SHAPE, lambda: lib.me_op_fov_add(h, ptr(a), ptr(a), ptr(b), 1, 8, 8, 64)),                    # tpw < g * g + 1
        (BAD_SHAPE, lambda: lib.me_op_fov_final(h, ptr(b), ptr(a), ptr(a), None, ptr(a), 1, 0, 8)),
        (BAD_ARG, lambda: lib.me_op_fov_final(h, ptr(b), ptr(a), ptr(a), None, None, 1, 2, 8)),
        (BAD_SHAPE, lambda: lib.me_op_nchw32_to_nhwc(h, ptr(a), ptr(a), None, 1, 0, 4, 8, 0, 0, 0)),
        (BAD_ARG, lambda: lib.me_op_nchw32_to_nhwc(h, ptr(a), ptr(a), None, 1, 4, 4, 8, 1, 0, 0)),         # a border without dst16
        (BAD_SHAPE, lambda: lib.me_op_nhwc16_to_nchw32(h, ptr(b), ptr(a), 1, 4, 4, 0, 0, 0)),
        (BAD_SHAPE, lambda: lib.me_op_patch_embed(h, ptr(b), 1, 8, 6, ptr(c), ptr(a), ptr(a), ptr(a), -1)),  # N % 4
        (BAD_ARG, lambda: lib.me_op_patch_embed(h, ptr(b), 1, 8, 8, ptr(c), None, ptr(a), ptr(a), -1)),
        (BAD_SHAPE, lambda: lib.me_op_cast_to16(h, ptr(a), ptr(b), 6)),
    ]
    for i, (code, launch) in enumerate(cases):
        rc = launch()
        assert rc == code, f"case {i}: returned {rc}, expected {code}: {lib.me_last_error(h)}"
        assert lib.me_last_error(h)
    ctx.synchronize()
    assert bool((a == 0).all()) and bool((b == 0).all()) and bool((c == 0).all())      # nothing was launched
    # the context works afterwards
    v = values((4096,), 9)
    vd = v.cuda()
    o = torch.empty(4096, dtype=torch.float16, device="cuda")
    call(ctx, lib.me_op_cast_to16, ptr(vd), ptr(o), 4096)
    same_bits(o, v.to(torch.float16))
    ctx.status_flags()
