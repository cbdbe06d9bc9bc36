"""Kernel-level tests (-m gpu) of the chained ConvTranspose launch -- two ConvTranspose2d(2, 2, stride 2) over one input grid
summed in ONE accumulator (csrc/gemm_core.h gemm_pp_kernel<..., CHAIN>, GemmParams::A2) -- through
me_op_conv_transpose2x2_pair, and of operand rows whose third part is read from the first (GemmParams::a_wrap) through
me_op_conv_transpose2x2_forms_wrap; then the two switches of the pipeline (ME_ENC0_SUM, ME_A_WRAP) on the tiny model.

What is held, and to what:
  * the 16-bit output of the pair is the 16-bit output of me_op_conv_transpose2x2_forms on set a alone BIT FOR BIT (same
    accumulator, same K order, zero start, no bias), its zero border included;
  * on small-integer operands -- every product and partial sum exact in f32 -- the f32 output is out32(a) + out32(b) of the two
    single launches bit for bit;
  * on random operands the f32 output is within test_gpu_ops.py test_conv_transpose's bound of the fp64 sum (max |err| / rms
    < 2e-5), and so is the sum of the two single launches on the same operands;
  * [hi | lo | hi] rows with the third part stored, and [hi | lo] rows with the wrap, give the same bits on every tile
    configuration a ConvTranspose can run on;
  * a chained descriptor on any tile configuration but 0 is ME_ERR_BAD_ARG.

Shapes: one 256 x 256 tile with 2 + 3 K slabs (8 x 8, 128 + 192 -> 64); a non-square 18 x 22 map of two images with two column
tiles, a ragged last row tile and an image boundary inside a tile (128 = [hi | lo] of 64, 192 = [hi | lo | hi] of 64 wrapped,
-> 128); the same map with four images under a grid cap of 8 workgroups (14 tiles: workgroups with one tile and with two)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import layout_refs as R
import matrix_eyes_amd as m
from matrix_eyes_amd.synthetic import synthetic_images
from oracle import depth_pro_oracle as O
from util import TORCH16, ctx_for, depth_error_report, max_abs_rel, oracle_cfg, pack_convt, ptr, rel_l2, weights_for

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SENT = -7.5
GUARD = 4096
BOUND = 2e-5          # test_gpu_ops.py test_conv_transpose: max |err| / rms(ref) of the f32 output
BAD_ARG = 1
RELU = 2
# name -> (B, H, W, K of set a, parts of set a, K of set b, parts of set b (3: [hi | lo | hi], stored wrapped), Cout, grid_cap)
SHAPES = {
    "one_tile": (1, 8, 8, 128, 1, 192, 1, 64, 0),
    "ragged": (2, 18, 22, 128, 2, 192, 3, 128, 0),
    "capped": (4, 18, 22, 128, 2, 192, 3, 128, 8),
}


def call(ctx, fn, *args):
    """One launch on the context's stream, fenced on both sides: the buffers were filled on torch's stream."""
    torch.cuda.synchronize()
    ctx._check(fn(ctx.handle, *args))
    ctx.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), f"{tag}: {int(ne.sum())} of {ne.numel()} elements differ"


def operand(g, M, K, parts, T, integer):
    """[M][K] 16-bit rows of `parts` K / parts-wide parts: 1 plain, 2 [hi | lo], 3 [hi | lo | hi] of an f32 value; integer: small
    integers instead (every product and every partial sum of the launch exact in f32), the part structure kept."""
    C = K // parts
    if integer:
        hi = torch.randint(-2, 3, (M, C), generator=g).to(T)
        lo = torch.randint(-1, 2, (M, C), generator=g).to(T)
    else:
        hi, lo = R.split_hi_lo(torch.randn(M, C, generator=g), T)
    return {1: hi, 2: torch.cat([hi, lo], -1), 3: torch.cat([hi, lo, hi], -1)}[parts].contiguous()


def weights(g, K, Cout, T, integer):
    """packed [(dy * 2 + dx) * Cout + co][K]: an independent ConvTranspose kernel per K column, whatever the parts mean"""
    if integer:
        w = torch.randint(-2, 3, (K, Cout, 2, 2), generator=g).float()
    else:
        w = torch.randn(K, Cout, 2, 2, generator=g) / math.sqrt(K)
    return pack_convt(w).to(T).contiguous()


def shuffle(rows, B, H, W, Cout):
    """[B * H * W][4 * Cout] GEMM rows -> [B][2H][2W][Cout]: column (dy * 2 + dx) * Cout + co of pixel (y, x) is (2y + dy, 2x + dx, co)"""
    return rows.reshape(B, H, W, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, Cout)


class Case:
    """The operands of one shape on the device, the two single launches' outputs and the fp64 sum: built once per (shape, dtype,
    integer) and shared by the tests, which leave it unchanged."""

    def __init__(self, ctx, dtype, shape, integer):
        self.ctx, self.T = ctx, TORCH16[dtype]
        self.B, self.H, self.W, self.Ka, self.pa, self.Kb, self.pb, self.Cout, self.cap = SHAPES[shape]
        self.tag = f"{shape} {dtype} {'integer' if integer else 'random'}"
        B, H, W, Cout, T = self.B, self.H, self.W, self.Cout, self.T
        M = B * H * W
        g = torch.Generator().manual_seed(1234 + 17 * len(shape) + (1 if integer else 0))
        Aa, Ab = operand(g, M, self.Ka, self.pa, T, integer), operand(g, M, self.Kb, self.pb, T, integer)
        Wa, Wb = weights(g, self.Ka, Cout, T, integer), weights(g, self.Kb, Cout, T, integer)
        bias = torch.randint(-3, 4, (Cout,), generator=g).float() if integer else torch.randn(Cout, generator=g)
        self.wrap = 2 * self.Kb // 3 if self.pb == 3 else 0                 # the stored width of set b's rows
        self.Aa, self.Wa, self.Wb, self.bias = Aa.cuda(), Wa.cuda(), Wb.cuda(), bias.cuda()
        self.Ab_full = Ab.cuda()
        self.Ab = Ab[:, :self.wrap].contiguous().cuda() if self.wrap else self.Ab_full
        ref = Aa.double() @ Wa.double().T + Ab.double() @ Wb.double().T + bias.double().repeat(4)
        self.ref = shuffle(ref, B, H, W, Cout)
        # the two single launches on tile configuration 0: set a with both outputs, set b (its rows stored in full) with its bias
        self.a16, self.a32 = self.out16(), self.out32()
        call(ctx, ctx.lib.me_op_conv_transpose2x2_forms, ptr(self.Aa), B, H, W, self.Ka, ptr(self.Wa), Cout, None, ptr(self.a32),
             ptr(self.a16), 1, RELU, 0, 0, 0, 0)
        self.b32 = self.out32()
        call(ctx, ctx.lib.me_op_conv_transpose2x2_forms, ptr(self.Ab_full), B, H, W, self.Kb, ptr(self.Wb), Cout, ptr(self.bias),
             ptr(self.b32), None, 0, 0, 0, 0, 0, 0)

    def out16(self, fill=0.0):
        """[B][2H + 2][2W + 2][Cout] and a guard behind it; zero as the pipeline's buffers are, unless the test says otherwise"""
        n = self.B * (2 * self.H + 2) * (2 * self.W + 2) * self.Cout
        buf = torch.full((n + GUARD,), SENT, dtype=self.T, device="cuda")
        buf[:n] = fill
        return buf

    def out32(self):
        return torch.full((self.B * 4 * self.H * self.W * self.Cout + GUARD,), SENT, dtype=torch.float32, device="cuda")

    def pair(self, o32, o16, tile_cfg=0, check=True):
        torch.cuda.synchronize()
        rc = self.ctx.lib.me_op_conv_transpose2x2_pair(self.ctx.handle, self.B, self.H, self.W, self.Cout, ptr(self.Aa), self.Ka, ptr(self.Wa),
                                                       ptr(self.Ab), self.Kb, self.wrap, ptr(self.Wb), ptr(self.bias), ptr(o32), ptr(o16), 1, RELU,
                                                       self.cap, tile_cfg)
        if check:
            self.ctx._check(rc)
        self.ctx.synchronize()
        return rc

    def map16(self, buf):
        return buf[:-GUARD].reshape(self.B, 2 * self.H + 2, 2 * self.W + 2, self.Cout)

    def map32(self, buf):
        return buf[:-GUARD].reshape(self.B, 2 * self.H, 2 * self.W, self.Cout)

    def check_frame(self, o32, o16, border_value):
        assert bool((o16[-GUARD:] == SENT).all()) and bool((o32[-GUARD:] == SENT).all()), f"{self.tag}: wrote behind an output"
        img = self.map16(o16)
        frame = torch.ones(img.shape[:3], dtype=torch.bool, device="cuda")
        frame[:, 1:-1, 1:-1] = False
        assert bool((img[frame] == border_value).all()), f"{self.tag}: wrote into the border"


_CASES = {}


def case_for(dtype, shape, integer):
    key = (dtype, shape, integer)
    if key not in _CASES:
        _CASES[key] = Case(ctx_for("tiny", dtype), dtype, shape, integer)
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pair_on_integers_is_the_exact_sum(dtype, shape):
    """Small-integer operands: out16 is set a's own 16-bit output bit for bit (ReLU'd, zero border), out32 is
    out32(a) + out32(b) of the two single launches bit for bit."""
    c = case_for(dtype, shape, True)
    assert float(c.ref.abs().max()) < 2 ** 20          # (far inside f32's exact integers: no partial sum can round)
    o32, o16 = c.out32(), c.out16()
    assert c.ctx.status_flags() == 0
    c.pair(o32, o16)
    assert c.ctx.status_flags() == 0
    c.check_frame(o32, o16, 0.0)
    same_bits(o16, c.a16, c.tag + " out16")
    same_bits(c.map32(o32), c.map32(c.a32) + c.map32(c.b32), c.tag + " out32")
    same_bits(c.map32(o32).cpu(), c.ref.float(), c.tag + " out32 against fp64")
    assert bool((c.map16(o16) >= 0).all()) and bool((c.map16(o16) > 0).any()) and bool((c.map32(o32) < 0).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pair_on_random_operands(dtype, shape):
    """Random operands: the same bit identity of the 16-bit output; the f32 output against the fp64 sum within the
    ConvTranspose test's bound, and the two-launch sum on the same operands within the same bound."""
    c = case_for(dtype, shape, False)
    o32, o16 = c.out32(), c.out16()
    c.pair(o32, o16)
    assert c.ctx.status_flags() == 0
    c.check_frame(o32, o16, 0.0)
    same_bits(o16, c.a16, c.tag + " out16")
    chained = max_abs_rel(c.map32(o32).cpu(), c.ref)
    two = max_abs_rel((c.map32(c.a32) + c.map32(c.b32)).cpu(), c.ref)
    print(f"{c.tag}: max_abs_rel against fp64: one accumulator {chained:.2e}, two launches {two:.2e}")
    assert chained < BOUND and two < BOUND, c.tag


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_pair_launches_in_a_row(dtype):
    """The same launch twice into the same buffers, sentinel-filled borders this time: the second finds the first's results and
    leaves the same bits; nothing but the outputs' pixels is written."""
    c = case_for(dtype, "ragged", False)
    o32, o16 = c.out32(), c.out16(SENT)
    c.pair(o32, o16)
    first32, first16 = o32.clone(), o16.clone()
    c.pair(o32, o16)
    c.check_frame(o32, o16, SENT)
    same_bits(o32, first32, c.tag + " out32 again")
    same_bits(o16, first16, c.tag + " out16 again")
    same_bits(c.map16(o16)[:, 1:-1, 1:-1], c.map16(c.a16)[:, 1:-1, 1:-1], c.tag + " out16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_is_refused_on_other_tiles(dtype):
    """Only tile configuration 0 has the chained form: every other id -- the automatic choice at this size included, which is the
    64 x 64 tile -- answers ME_ERR_BAD_ARG and writes nothing."""
    c = case_for(dtype, "one_tile", False)
    o32, o16 = c.out32(), c.out16(SENT)
    for cfg in [-1] + list(range(1, 14)):
        assert c.pair(o32, o16, cfg, check=False) == BAD_ARG, cfg
    assert bool((o32 == SENT).all()) and bool((o16 == SENT).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_wrapped_third_part_changes_no_bit(dtype, cfg):
    """[hi | lo | hi] rows stored in full through me_op_conv_transpose2x2_forms, and the same rows stored [hi | lo] with the third
    part read from the first (me_op_conv_transpose2x2_forms_wrap): the same bits in both outputs, on every tile configuration
    a ConvTranspose runs on."""
    c = case_for(dtype, "ragged", False)
    ctx, B, H, W, Cout = c.ctx, c.B, c.H, c.W, c.Cout
    outs = []
    for wrap in (0, c.wrap):
        o32, o16 = c.out32(), c.out16()
        A = c.Ab if wrap else c.Ab_full
        if wrap:
            call(ctx, ctx.lib.me_op_conv_transpose2x2_forms_wrap, ptr(A), B, H, W, c.Kb, wrap, ptr(c.Wb), Cout, ptr(c.bias), ptr(o32), ptr(o16),
                 1, RELU, 0, 0, 0, cfg)
        else:
            call(ctx, ctx.lib.me_op_conv_transpose2x2_forms, ptr(A), B, H, W, c.Kb, ptr(c.Wb), Cout, ptr(c.bias), ptr(o32), ptr(o16),
                 1, RELU, 0, 0, 0, cfg)
        c.check_frame(o32, o16, 0.0)
        outs.append((o32, o16))
    same_bits(outs[1][0], outs[0][0], f"{c.tag} cfg {cfg} out32")
    same_bits(outs[1][1], outs[0][1], f"{c.tag} cfg {cfg} out16")
    if cfg == 0:
        same_bits(outs[0][0], c.b32, c.tag + " the case's own launch")


def test_wrap_is_checked():
    """a_wrap: a multiple of 64 that leaves no more channels behind it than stand before it"""
    c = case_for("f16", "one_tile", False)
    o32 = c.out32()
    for wrap in (32, 64, 192, 256, -64):
        rc = c.ctx.lib.me_op_conv_transpose2x2_forms_wrap(c.ctx.handle, ptr(c.Ab_full), c.B, c.H, c.W, c.Kb, wrap, ptr(c.Wb), c.Cout, None,
                                                          ptr(o32), None, 0, 0, 0, 0, 0, 0)
        assert rc != 0, wrap
    assert bool((o32 == SENT).all())


_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import matrix_eyes_amd as m
from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
cfg = m.ModelConfig.tiny()
ctx = m.Context(0, "f16", cfg)
ctx.load_state_dict(synthetic_checkpoint(cfg))
rgb = synthetic_images(2, cfg.img_size, "structured", seed=5)
d, fov = ctx.extract_depth(rgb, None, want_fov=True)
again, fov2 = ctx.extract_depth(rgb, None, want_fov=True)
assert np.array_equal(d, again) and np.array_equal(fov, fov2)
one, _ = ctx.extract_depth(rgb[1:], None, want_fov=True)      # a batch stays a loop of batch-one calls
assert np.array_equal(d[1], one[0])
np.save(sys.argv[2], d)
"""


def test_tiny_model_switches(tmp_path):
    """The tiny model in child processes (the switches are read once per process): all three parts stored and two launches
    (ME_A_WRAP=0 ME_ENC0_SUM=0), the wrap alone (ME_ENC0_SUM=0), and the default with the chained launch in front of level 0.
    The wrap changes no bit of the depth.  The chained sum rounds x0 + x1 once instead of twice -- another realisation of the same
    rounding noise, held to the 1.5e-3 test_gpu_pipeline.py test_tile_choices_change_no_bit holds such a change to -- and every
    run is within the tiny model's oracle tolerance (test_gpu_pipeline.py test_extract_depth_tiny: 2e-3).  ME_LOG_LAUNCH shows
    which launches ran."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for name, extra in (("stored", {"ME_A_WRAP": "0", "ME_ENC0_SUM": "0"}), ("wrapped", {"ME_ENC0_SUM": "0"}), ("chained", {})):
        path = str(tmp_path / (name + ".npy"))
        env = {k: v for k, v in os.environ.items() if k not in ("ME_A_WRAP", "ME_ENC0_SUM")}
        r = subprocess.run([sys.executable, "-c", _CHILD, root, path], env=dict(env, ME_LOG_LAUNCH="1", **extra), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        convt = [ln for ln in r.stderr.splitlines() if ln.startswith("gemm_launch plain convt")]
        runs[name] = (np.load(path), any(" wrap=8 " in ln for ln in convt), any(ln.rstrip().endswith("K2=768") for ln in convt))
    assert (runs["stored"][1], runs["stored"][2]) == (False, False)
    assert (runs["wrapped"][1], runs["wrapped"][2]) == (True, False)
    assert runs["chained"][2]
    assert np.array_equal(runs["wrapped"][0], runs["stored"][0])
    moved = rel_l2(runs["chained"][0], runs["stored"][0])
    cfg = m.ModelConfig.tiny()
    rgb = synthetic_images(2, cfg.img_size, "structured", seed=5)
    ref, _ = O.extract_depth(O.preprocess_u8(rgb), None, weights_for("tiny"), oracle_cfg(cfg))
    errs = {name: depth_error_report(d, ref.numpy())["rel_l2"] for name, (d, _, _) in runs.items()}
    print(f"chained against two launches: rel-L2 {moved:.2e}; against the oracle: {errs}")
    assert np.isfinite(runs["chained"][0]).all() and moved < 1.5e-3
    assert all(e < 2e-3 for e in errs.values()), errs
