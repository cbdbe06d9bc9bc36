"""The table of model configurations that tests/test_config_sweep_cpu.py (admission + coverage, no GPU) and
tests/test_gpu_config_sweep.py (the HIP path against the fp32 oracle) share.  A plain module: no test lives here.

me_ctx_create admits grid 8..64, embed_dim 64..1024, depth 1..64, any two distinct tap blocks, enc_dims in multiples of
64, dec_dim in multiples of 256, head_dims[0] in multiples of 4 up to 32 and sixteen split_operands masks; the pipeline
picks kernels, tiles, fusions and buffer sizes from those numbers.  Each case below is one point of that space chosen so
that dimensions which are EQUAL in ModelConfig.tiny() and ModelConfig() (enc_dims[2] == enc_dims[3], head_dims[0] == 32,
ascending taps, dec_dim 256) differ, at sizes the CPU oracle finishes in seconds.  test_config_sweep_cpu.py asserts the
coverage conditions over the table, so an edit cannot drop one silently.

split_operands bits (csrc/model.h): 1 upsample, 2 fusion out, 4 head (set: the composed head is OFF), 8 decoder convs."""
from dataclasses import dataclass
from typing import Tuple

import matrix_eyes_amd as m

# the project's own bounds (tests/test_gpu_pipeline.py TOL and the multipliers of test_stages_tiny / test_extract_depth_tiny)
TOL = {"f16": 1.0e-3, "bf16": 8.0e-3}
ENC_MULT, E2E_MULT = 1.5, 2.0
FOV_TOL_DEG = {"f16": 0.05, "bf16": 0.05 * 8}
# share of a bound that the reference's own sensitivity to 16-bit operand rounding (OracleConfig.operand_dtype) may take
FLOOR_SHARE = {"f16": 0.8, "bf16": 0.95}

SPLIT_HEAD = 4


@dataclass(frozen=True)
class Case:
    name: str
    cfg: m.ModelConfig
    ckpt_seed: int = 2024
    family: str = "structured"
    img_seed: int = 4321
    batch: int = 1
    vit_entry: bool = False
    bf16: bool = False
    ln_unfused_child: bool = False      # also run in a child process with ME_LN_FUSE=0

    @property
    def dtypes(self) -> Tuple[str, ...]:
        return ("f16", "bf16") if self.bf16 else ("f16",)

    @property
    def composed_head(self) -> bool:
        return not (self.cfg.split_operands & SPLIT_HEAD)


def _cfg(grid=8, C=128, depth=4, taps=(1, 2), enc=(64, 128, 128, 128), dec=256, head=32, mask=3, eps=1e-5, align=True):
    return m.ModelConfig(grid=grid, embed_dim=C, num_heads=C // 64, depth=depth, tap_blocks=taps, enc_dims=enc, dec_dim=dec,
                         head_dims=(head, 1), ln_eps=eps, align_corners=align, split_operands=mask)


CASES = [
    Case("tiny", _cfg(), bf16=True, vit_entry=True),
    Case("tiny_head16", _cfg(head=16), ckpt_seed=3, batch=2, bf16=True),
    Case("tiny_head4_mask0", _cfg(head=4, mask=0, enc=(64, 128, 192, 256)), img_seed=5),
    Case("c64_d2_taps_desc", _cfg(C=64, depth=2, taps=(1, 0), mask=0), batch=3, family="noise", img_seed=1234),
    Case("c128_d5_enc_mixed_head24", _cfg(depth=5, taps=(4, 0), enc=(128, 64, 256, 192), head=24, eps=1e-6, align=False, mask=5),
         batch=2, family="noise", img_seed=77),
    Case("c256", _cfg(C=256), vit_entry=True, bf16=True, ln_unfused_child=True),
    Case("c256_d5_head8_mask10", _cfg(C=256, depth=5, taps=(2, 4), enc=(64, 192, 128, 256), head=8, mask=10), ckpt_seed=7),
    Case("c512_d3_head8", _cfg(C=512, depth=3, taps=(0, 2), enc=(128, 64, 192, 128), head=8), batch=2),
    Case("c512_d2_mask15", _cfg(C=512, depth=2, taps=(0, 1), head=4, mask=15, eps=1e-6)),
    Case("dec512", _cfg(dec=512, mask=10)),
    Case("dec512_head24_mask15", _cfg(dec=512, head=24, mask=15, enc=(64, 128, 192, 256), align=False), ckpt_seed=5),
    Case("grid16_c128_d3", _cfg(grid=16, depth=3, taps=(0, 1), enc=(64, 128, 192, 256)), ckpt_seed=3, img_seed=9),
    Case("grid16_c256_d2", _cfg(grid=16, C=256, depth=2, taps=(1, 0), enc=(64, 192, 128, 256), head=16), vit_entry=True),
    Case("grid24_c64_d2", _cfg(grid=24, C=64, depth=2, taps=(0, 1), enc=(64, 128, 192, 256), mask=5)),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# (case, dtype) pairs in table order: the ids of both parametrised tests
PAIRS = [(c.name, d) for c in CASES for d in c.dtypes]


def weights_of(case: Case):
    from matrix_eyes_amd.synthetic import synthetic_checkpoint
    return synthetic_checkpoint(case.cfg, seed=case.ckpt_seed)


def images_of(case: Case):
    """u8 [batch, S, S, 3]"""
    from matrix_eyes_amd.synthetic import synthetic_images
    return synthetic_images(case.batch, case.cfg.img_size, case.family, seed=case.img_seed)


_REF = {}


def reference(name: str):
    """(weights, image f32 [B,3,S,S], inverse depth, fov_deg, parts) of the fp32 oracle for a case; the last case asked for is
    kept, so that the operand types of one case (consecutive in PAIRS) share the pass."""
    if name not in _REF:
        from oracle import depth_pro_oracle as O
        from util import oracle_cfg
        _REF.clear()
        case = BY_NAME[name]
        w = weights_of(case)
        img = O.preprocess_u8(images_of(case))
        inv, fov, parts = O.extract_depth(img, None, w, oracle_cfg(case.cfg), return_parts=True)
        _REF[name] = (w, img, inv, fov, parts)
    return _REF[name]
