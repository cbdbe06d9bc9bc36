"""CPU tests of tests/layout_refs.py: the plain references that test_gpu_layout.py and test_gpu_split_forms.py hold
the HIP kernels to are themselves tied to oracle/depth_pro_oracle.py here, so the GPU tests do not rest on a second,
unverified copy of the window geometry; and the three facts about the [hi | lo] split that the GPU tests use as
constants are asserted on 10 M values."""
import math

import pytest
import torch
import torch.nn.functional as F

import layout_refs as R
from oracle import depth_pro_oracle as O

GRIDS = [8, 16, 24, 32, 40, 48, 56, 64]       # every grid me_ctx_create admits


def _oracle_order(t, batch, wpi, win0, n):
    """Windows win0 .. win0 + n - 1 of each image out of an image-major stack [batch * wpi][...], in the oracle's
    order (window-major: encoder.rs split concatenates whole batches window by window)."""
    return torch.stack([t[b * wpi + win0 + i] for i in range(n) for b in range(batch)])


@pytest.mark.parametrize("grid", GRIDS)
def test_merge_is_the_oracles(grid):
    batch, C = 2, 8
    P = grid * grid
    g = torch.Generator().manual_seed(grid)
    tok = torch.randn(batch * 35, P + 1, C, generator=g)
    for steps, padding, win0 in ((5, grid // 8, 0), (3, grid // 4, 25), (1, 0, 34)):
        wins = _oracle_order(tok, batch, 35, win0, steps * steps)
        want = O.merge(O.reshape_feature(wins, grid, grid, 1), batch, padding)              # NCHW
        got = R.merge(tok, batch, 35, win0, steps, padding, grid)
        side = grid if steps == 1 else 2 * (grid - padding) + (steps - 2) * (grid - 2 * padding)
        assert got.shape == (batch, side, side, C)
        assert torch.equal(R.nhwc_to_nchw(got), want), (steps, padding)
    # one window per image (the image encoder's map): wpi 1, win0 0
    tok1 = torch.randn(batch, P + 1, C, generator=g)
    want = O.merge(O.reshape_feature(tok1, grid, grid, 1), batch, 0)
    assert torch.equal(R.nhwc_to_nchw(R.merge(tok1, batch, 1, 0, 1, 0, grid)), want)


@pytest.mark.parametrize("grid,align", [(8, True), (8, False), (16, True)])
def test_patchify_rows_are_the_oracles_im2col(grid, align):
    batch, C = 2, 24
    P, wp = grid * grid, 16 * grid
    g = torch.Generator().manual_seed(100 + grid)
    x = torch.randn(batch, 3, 4 * wp, 4 * wp, generator=g)
    cfg = O.OracleConfig(grid=grid, embed_dim=C, align_corners=align, dtype=torch.float64)
    x0, x1, x2 = O.create_pyramid(x, cfg)
    owins = torch.cat([O.split(x0, 4, wp), O.split(x1, 2, wp), x2], dim=0)          # 25 B + 9 B + B, window-major
    assert owins.shape[0] == 35 * batch
    # the same windows image-major, as the kernels index them
    mine = R.windows_of(x0, x1, x2, grid)
    order = [w * batch + b for b in range(batch) for w in range(35)]
    assert torch.equal(mine, owins[order])
    patches = R.patchify(x0, x1, x2, grid)
    assert patches.shape == (batch * 35 * P, 768)
    # column order c * 256 + iy * 16 + ix: exactly torch's unfold
    unf = F.unfold(mine, 16, stride=16).transpose(1, 2).reshape(-1, 768)
    assert torch.equal(patches, unf)
    assert torch.equal(R.patchify_windows(x2, grid), patches.reshape(batch, 35, P, 768)[:, 34].reshape(-1, 768))
    # ... and patches . W^T + b is the oracle's patch embedding; with cls and pos, its token stream (fp64: the
    # two differ in summation order only)
    w = torch.randn(C, 3, 16, 16, generator=g, dtype=torch.float64) / math.sqrt(768)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    cls = torch.randn(1, 1, C, generator=g, dtype=torch.float64)
    pos = torch.randn(1, P + 1, C, generator=g, dtype=torch.float64)
    weights = {"patch_embed.proj.weight": w, "patch_embed.proj.bias": b, "cls_token": cls, "pos_embed": pos}
    want = O.patch_embed_forward(mine.double(), weights, "patch_embed.", cfg)
    got = (patches.double() @ w.reshape(C, 768).T + b).reshape(batch * 35, P, C)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max()) * 768
    want_tok = O.prepare_tokens_with_mask(mine.double(), weights, "", cfg)
    got_tok = R.patch_embed_tokens(patches, w.reshape(C, 768), b, pos[0], cls[0, 0], P)
    assert float((got_tok - want_tok).abs().max()) < 1e-12 * float(want_tok.abs().max()) * 768
    # cls_rows: row 0 only
    t = torch.randn(3, P + 1, C, generator=g)
    c32, p32 = cls[0, 0].float(), pos[0].float()
    out = R.cls_rows(t, c32, p32)
    assert torch.equal(out[:, 1:], t[:, 1:]) and torch.equal(out[:, 0], (c32 + p32[0]).expand(3, C))
    assert float((out[:, 0].double() - want_tok[:3, 0]).abs().max()) < 2.0 ** -22 * float(want_tok[:, 0].abs().max())


def test_fov_add_is_the_oracles_reshape():
    B, grid, C = 3, 8, 16
    g = torch.Generator().manual_seed(5)
    lin = torch.randn(B, grid * grid + 1, C, generator=g)
    low_nchw = torch.randn(B, C, grid, grid, generator=g)
    want = lin[:, 1:, :].permute(0, 2, 1).reshape(low_nchw.shape) + low_nchw            # fov.rs:66-74 as the oracle writes it
    low = R.nchw_to_nhwc(low_nchw).reshape(B, grid * grid, C)
    assert torch.equal(R.nhwc_to_nchw(R.fov_add(lin, low, grid)), want)


def test_layout_changes_and_concat():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 5, 3, 7, generator=g)
    n = R.nchw_to_nhwc(x)
    assert n.shape == (2, 3, 7, 5) and n[1, 2, 6, 4] == x[1, 4, 2, 6] and torch.equal(R.nhwc_to_nchw(n), x)
    canvas = torch.full((2, 5, 9, 5), -7.0)
    bd = R.into_border(canvas, n)
    assert torch.equal(bd[:, 1:-1, 1:-1], n)
    edge = torch.ones(2, 5, 9, dtype=torch.bool)
    edge[:, 1:-1, 1:-1] = False
    assert bool((bd[edge] == -7.0).all())
    a, b = torch.randn(4, 8, generator=g), torch.randn(4, 16, generator=g)
    c = R.concat_channels(a, b)
    assert torch.equal(c[:, :8], a) and torch.equal(c[:, 8:], b)
    sp = R.split_pixels(n, torch.float16)
    hi, lo = R.split_hi_lo(n, torch.float16)
    assert sp.shape == (2, 3, 7, 10) and torch.equal(sp[..., :5], hi) and torch.equal(sp[..., 5:], lo)


def test_hi_lo_split_facts():
    """10 M magnitudes log-uniform over 1e-9 .. 7e4, both signs, plus the edges: the f32 subtraction v - hi is exact;
    |hi + lo - v| <= 2^-22 |v| for f16 where |v| >= 2^-3 and <= 2^-25 absolute below that; <= 2^-16 |v| for bf16."""
    g = torch.Generator().manual_seed(7)
    n = 10_000_000
    mag = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(math.log(1e-9), math.log(7e4), generator=g))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    edges = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65519.996, 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 1.0 + 2.0 ** -11,
                          1.0 + 3 * 2.0 ** -11, 2.0 ** -3, 0.125 - 2.0 ** -14], dtype=torch.float64)
    v = torch.cat([(mag * sign), edges]).float()
    vd = v.double()
    for T in (torch.float16, torch.bfloat16):
        hi, lo = R.split_hi_lo(v, T)
        fin = torch.isfinite(hi)
        assert bool((lo[~fin] == 0).all()) and bool(torch.isinf(hi[~fin]).all())
        if T == torch.bfloat16:
            assert bool(fin.all())
        else:
            assert bool((vd[~fin].abs() >= 65520).all()) and bool((vd[fin].abs() < 65520).all())
        d32 = (v - hi.float())[fin]
        assert torch.equal(d32.double(), (vd - hi.double())[fin]), "the f32 subtraction is exact"
        err = (hi.double() + lo.double() - vd).abs()[fin]
        a = vd.abs()[fin]
        if T == torch.float16:
            big = a >= 2.0 ** -3
            assert bool((err[big] <= R.SPLIT_REL[T] * a[big]).all())
            assert bool((err[~big] <= R.SPLIT_ABS_F16).all())
        else:
            assert bool((err <= R.SPLIT_REL[T] * a).all())
        # |lo| <= ulp(hi) / 2, the structural bound the GPU tests assert on kernel outputs
        assert bool((lo.double().abs()[fin] <= R.ulp16(hi)[fin] / 2).all())
    # an overflowed hi keeps lo = 0 and its sign
    hi, lo = R.split_hi_lo(torch.tensor([7e4, -7e4]), torch.float16)
    assert hi.tolist() == [math.inf, -math.inf] and lo.tolist() == [0.0, 0.0]
