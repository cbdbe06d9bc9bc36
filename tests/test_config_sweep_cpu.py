"""The configuration sweep, CPU side (no GPU): (a) OracleConfig.operand_dtype leaves the default oracle alone, (b) every case
of tests/config_sweep_cases.py is ADMITTED -- the fp32 oracle against itself with 16-bit operand rounding stays inside a fixed
share of each bound the GPU test holds the HIP path to -- and (c) the table covers the dimensions it was written to cover.

(b) is not a model of the HIP path (which carries f32 accumulators, an f32 residual stream and hi + lo operands in places): it
measures, from the reference alone, how far 16-bit operand rounding moves each asserted quantity for this configuration,
checkpoint seed and image.  Where that alone takes the bound (a map the closing ReLU has mostly zeroed inflates every relative
figure), a failure of the GPU test would say nothing about the kernels: such a case gets other seeds or another depth / width,
never another bound."""
import pytest
import torch

from oracle import depth_pro_oracle as O
from config_sweep_cases import (BY_NAME, CASES, E2E_MULT, ENC_MULT, FLOOR_SHARE, FOV_TOL_DEG, PAIRS, SPLIT_HEAD, TOL,
                                reference)
from util import oracle_cfg, rel_l2

ROUND = {"f16": torch.float16, "bf16": torch.bfloat16}


def _reference(name):
    return reference(name)


def floors(name, dtype):
    """What the GPU test asserts, formed the same way (each stage fed the fp32 oracle's own inputs), with the rounded oracle
    in the place of the HIP path."""
    case = BY_NAME[name]
    w, img, inv, fov, parts = _reference(name)
    rcfg = oracle_cfg(case.cfg)
    rcfg.operand_dtype = ROUND[dtype]
    with torch.no_grad():
        r_inv, r_fov_e2e, r_parts = O.extract_depth(img, None, w, rcfg, return_parts=True)
        r_feat, r_low = O.decoder_forward(parts["encodings"], w, rcfg)
        r_canon = O.head_forward(parts["features"], w, rcfg)
        r_fov = O.fov_forward(img, parts["lowres"], w, rcfg)
    return {
        "encodings": max(rel_l2(a, b) for a, b in zip(r_parts["encodings"], parts["encodings"])),   # the encoder's input is the image
        "features": rel_l2(r_feat, parts["features"]),
        "lowres": rel_l2(r_low, parts["lowres"]),
        "canonical": rel_l2(r_canon, parts["canonical"]),
        "fov_deg": float((r_fov - fov).abs().max()),
        "fov_deg_e2e": float((r_fov_e2e - fov).abs().max()),
        "depth_e2e": rel_l2(r_inv, inv),
        "at_clamp": float((inv <= 1e-4).float().mean()),
    }


def bounds(dtype):
    t = TOL[dtype]
    return {"encodings": ENC_MULT * t, "features": t, "lowres": t, "canonical": t, "fov_deg": FOV_TOL_DEG[dtype],
            "fov_deg_e2e": FOV_TOL_DEG[dtype], "depth_e2e": E2E_MULT * t}


@pytest.mark.parametrize("name,dtype", PAIRS, ids=[f"{n}-{d}" for n, d in PAIRS])
def test_case_is_admitted(name, dtype):
    got, lim = floors(name, dtype), bounds(dtype)
    print("floor", name, dtype, {k: "%.3g" % v for k, v in got.items()})
    for key, bound in lim.items():
        assert got[key] <= FLOOR_SHARE[dtype] * bound, (
            f"{name} [{dtype}] {key}: the reference alone moves by {got[key]:.3g} under operand rounding, more than "
            f"{FLOOR_SHARE[dtype]} x the bound {bound:.3g} ({got['at_clamp']:.0%} of the map at the clamp): re-seed or resize the case")


def test_operand_dtype_default_leaves_the_oracle_bit_for_bit():
    case = BY_NAME["tiny"]
    w, img, inv, fov, parts = _reference("tiny")
    cfg = oracle_cfg(case.cfg)
    assert cfg.operand_dtype is None and O.OracleConfig().operand_dtype is None
    x, wt = torch.randn(3, 8), torch.randn(5, 8)
    a, b = O._ops(cfg, x, wt)
    assert a is x and b is wt                         # the very tensors, not copies: nothing is rounded, nothing re-laid
    # the restated calls against torch.nn.functional called directly, the way the oracle called it before the field existed
    import torch.nn.functional as F
    xc, wc, bc = torch.randn(2, 8, 6, 6), torch.randn(4, 8, 3, 3), torch.randn(4)
    assert torch.equal(O._linear(cfg, x, wt, bc[:0].new_zeros(5)), F.linear(x, wt, torch.zeros(5)))
    assert torch.equal(O._conv2d(cfg, xc, wc, bc, padding=1), F.conv2d(xc, wc, bc, padding=1))
    wtr = torch.randn(8, 4, 2, 2)
    assert torch.equal(O._conv_transpose2d(cfg, xc, wtr, stride=2), F.conv_transpose2d(xc, wtr, stride=2))
    # rounding to the type the tensors already have is the identity: the whole model, every call site, same bits
    same = oracle_cfg(case.cfg)
    same.operand_dtype = torch.float32
    inv2, fov2, parts2 = O.extract_depth(img, None, w, same, return_parts=True)
    assert torch.equal(inv2, inv) and torch.equal(fov2, fov) and torch.equal(parts2["features"], parts["features"])
    assert all(torch.equal(p, q) for p, q in zip(parts2["encodings"], parts["encodings"]))
    # and a 16-bit type rounds BOTH operands of a call, nothing else
    half = oracle_cfg(case.cfg)
    half.operand_dtype = torch.float16
    assert torch.equal(O._linear(half, x, wt), F.linear(x.half().float(), wt.half().float()))
    assert torch.equal(O._conv2d(half, xc, wc, bc, padding=1), F.conv2d(xc.half().float(), wc.half().float(), bc, padding=1))
    assert torch.equal(O._conv_transpose2d(half, xc, wtr, stride=2),
                       F.conv_transpose2d(xc.half().float(), wtr.half().float(), stride=2))
    assert not torch.equal(O._linear(half, x, wt), F.linear(x, wt))


def test_table_covers_what_it_was_written_for():
    cfgs = [c.cfg for c in CASES]
    assert 12 <= len(CASES) <= 16

    def some(pred, at_least=1):
        return sum(1 for c in CASES if pred(c)) >= at_least

    # grid
    assert {c.grid for c in cfgs} == {8, 16, 24}
    g24 = [c for c in cfgs if c.grid == 24]
    assert len(g24) == 1 and g24[0].embed_dim == 64 and g24[0].depth == 2
    assert some(lambda c: c.cfg.grid == 16, 2) and some(lambda c: c.cfg.grid == 16 and c.cfg.embed_dim >= 256)
    # embed_dim: 1024 stays with the full-size tests
    assert {c.embed_dim for c in cfgs} == {64, 128, 256, 512}
    assert all(c.embed_dim == 64 * c.num_heads for c in cfgs)
    assert some(lambda c: c.cfg.embed_dim >= 256, 3)
    assert some(lambda c: c.cfg.embed_dim >= 256 and c.cfg.depth == 2) and some(lambda c: c.cfg.embed_dim >= 256 and c.cfg.depth >= 5)
    # tap blocks
    assert all(0 <= t < c.depth for c in cfgs for t in c.tap_blocks) and all(c.tap_blocks[0] != c.tap_blocks[1] for c in cfgs)
    assert some(lambda c: c.cfg.tap_blocks[0] > c.cfg.tap_blocks[1])
    assert some(lambda c: c.cfg.depth - 1 in c.cfg.tap_blocks) and some(lambda c: 0 in c.cfg.tap_blocks)
    # enc_dims
    distinct = [c.enc_dims for c in cfgs if len(set(c.enc_dims)) == 4]
    assert len(distinct) >= 4 and len({tuple(sorted(range(4), key=lambda i: e[i])) for e in distinct}) >= 2
    assert some(lambda c: c.cfg.enc_dims[2] > c.cfg.enc_dims[3]) and some(lambda c: c.cfg.enc_dims[0] > c.cfg.enc_dims[1])
    assert all(e % 64 == 0 for c in cfgs for e in c.enc_dims)
    # dec_dim, head_dims
    assert some(lambda c: c.cfg.dec_dim == 512) and some(lambda c: c.cfg.dec_dim == 256)
    assert {c.head_dims[0] for c in cfgs} == {4, 8, 16, 24, 32} and all(c.head_dims[1] == 1 for c in cfgs)
    assert some(lambda c: c.cfg.head_dims[0] < 32 and c.composed_head, 2)
    assert len({c.cfg.head_dims[0] for c in CASES if c.cfg.head_dims[0] < 32 and c.composed_head}) >= 2
    assert some(lambda c: c.cfg.head_dims[0] < 32 and not c.composed_head)
    assert all(c.composed_head == (not (c.cfg.split_operands & SPLIT_HEAD)) for c in CASES)
    # split_operands
    assert {0, 3, 5, 10, 15} <= {c.split_operands for c in cfgs}
    # the assumed semantics, outside tiny
    tiny = BY_NAME["tiny"].cfg
    assert some(lambda c: c.cfg.ln_eps == 1e-6 and c.cfg != tiny) and some(lambda c: not c.cfg.align_corners and c.cfg != tiny)
    # batch, image family
    assert {1, 2, 3} <= {c.batch for c in CASES} and {c.family for c in CASES} == {"structured", "noise"}
    # entry points and operand types
    vit = [c for c in CASES if c.vit_entry]
    assert len(vit) >= 3 and any(c.cfg.embed_dim >= 256 for c in vit) and any(c.cfg.grid == 16 for c in vit)
    bf = [c for c in CASES if c.bf16]
    assert len(bf) >= 3 and any(c.cfg.embed_dim >= 256 for c in bf) and any(c.cfg.head_dims[0] < 32 for c in bf)
    assert all(c.dtypes == (("f16", "bf16") if c.bf16 else ("f16",)) for c in CASES)
    assert sum(1 for c in CASES if c.ln_unfused_child) == 1 and all(c.cfg.embed_dim >= 256 for c in CASES if c.ln_unfused_child)
    # the baseline point itself is in the table, unchanged
    import matrix_eyes_amd as m
    assert tiny == m.ModelConfig.tiny()
