"""Exact-arithmetic checkpoints, shared by tests/test_exact_cpu.py (admission, coverage and sensitivity, no GPU) and
tests/test_gpu_exact.py (the HIP path against the fp32 oracle, bit for bit).  A plain module: no test lives here.

Every whole-model comparison of the suite is held at the size of the 16-bit rounding noise itself (config_sweep_cases.TOL), so a
wiring error worth a third of that passes.  Here the rounding is taken out of the experiment: weights and inputs are small
integers (sparse +-1 rows, biases in {-1, 0, 1}) for which every operand, product, partial sum and intermediate is exactly
representable in f16, bf16 and f32.  Operand rounding, the order of the f32 sums, hi + lo splitting (lo = 0), composing two
layers in f64 and skipping an intermediate rounding then change nothing, and the HIP path has to EQUAL the oracle.

What is exact: the decoder and the head on integer encodings (features, lowres, canonical), and the front of the encoder --
patch embedding, the ViT's residual stream through blocks that add a known integer vector each (their own: the output after
every block differs, so a mis-routed tap is an integer-sized error), the taps, merge, and the two
latent upsample stacks (encodings 0 and 1).  What is not: encodings 2-4 and the FOV head (the final LayerNorm and the bilinear
pyramid), so they are not compared.  qkv, the MLP and the norms keep their Gaussian values: attention, GELU and LayerNorm run
on real data and reach the residual stream through an all-zero projection (attention) or a zero LayerScale (the MLP).

End to end (cases with e2e): extract_depth(image, f_norm = 1) is the only entry that runs the composed features (weights.hip
compose_features, GemmParams::tap_bias) -- decoder_forward hands out the f32 feature map and so keeps the two layers apart.  It
is made exact by zero weights in the three coarse upsample stacks and fuse_lowres (COARSE_ZERO below).

The cases take their dimensions from config_sweep_cases.BY_NAME.  The two largest grids run the encoder entries only: what they
are in the table for (merge paddings 2 / 4 and 3 / 6, 257 and 577 tokens) is in the encoder, and the four oracle modes of their
decoder maps (512^2 and 768^2 x 256 channels) would add more than a minute to the CPU admission file, which is at its limit."""
from dataclasses import dataclass
from typing import Dict, Tuple

import torch

import matrix_eyes_amd as m
from matrix_eyes_amd.config import expected_weights
from matrix_eyes_amd.synthetic import synthetic_checkpoint
from oracle import depth_pro_oracle as O
from config_sweep_cases import BY_NAME
from util import oracle_cfg

# largest |value| that may enter a linear / convolution call: integers up to 2^(p) are exact with p significand bits
MAG_LIMIT = {"f16": 2048.0, "bf16": 256.0}
PATCH = "encoder.patch_encoder."
# the layers weights.hip composes at load time (compose_head, compose_features, out_conv o deconv): two nonzeros per row where
# the magnitudes allow it, so that a composed weight is a sum of products, not a single product
COMPOSED = ("head.0.weight", "head.1.weight", "head.2.weight", ".deconv.weight", ".out_conv.weight")
# Behind the final LayerNorm and the bilinear pyramid nothing is exact, so the three coarse upsample stacks and fuse_lowres get
# all-zero weights: end to end, encodings 2 and 3 are exactly zero and encoding 4 is fuse_lowres.bias at every pixel, while the
# two latents carry the image.  That makes extract_depth(image, f_norm = 1) exact
COARSE_ZERO = ("encoder.upsample0.", "encoder.upsample1.", "encoder.upsample2.", "encoder.fuse_lowres.weight")
VIT_WINDOWS = 5


@dataclass(frozen=True)
class ExactCase:
    name: str                       # key of config_sweep_cases.BY_NAME: dimensions, split mask and batch come from there
    seed: int
    # nonzeros per row of the COMPOSED layers of (the head, the decoder).  Two in the decoder's leave 99 % of the feature map
    # nonzero at magnitudes past 2^8, which the admission rule (test_exact_cpu.py) refuses: one is the fallback there
    nnz: Tuple[int, int] = (2, 1)
    bf16: bool = False
    decoder: bool = True            # False: encoder and ViT entries only (see the module text)
    e2e: bool = False               # also extract_depth(image, f_norm = 1): the one entry that runs compose_features / tap_bias
    children: Tuple[Tuple[str, str], ...] = ()      # (variable, value): the case again in a child process with it set

    @property
    def cfg(self) -> m.ModelConfig:
        return BY_NAME[self.name].cfg

    @property
    def batch(self) -> int:
        return BY_NAME[self.name].batch

    @property
    def dtypes(self) -> Tuple[str, ...]:
        return ("f16", "bf16") if self.bf16 else ("f16",)

    @property
    def limit(self) -> float:
        return MAG_LIMIT["bf16" if self.bf16 else "f16"]


_COMPOSED_OFF = (("ME_HEAD_COMPOSED", "0"), ("ME_FEAT_COMPOSED", "0"))

# seeds and nnz were chosen from the fp32 / fp64 oracle alone, by the conditions tests/test_exact_cpu.py asserts
EXACT = [
    ExactCase("tiny", seed=2, bf16=True, e2e=True, children=_COMPOSED_OFF),
    ExactCase("tiny_head16", seed=1, bf16=True, e2e=True, children=_COMPOSED_OFF),
    ExactCase("tiny_head4_mask0", seed=3, e2e=True),
    ExactCase("c64_d2_taps_desc", seed=1),
    ExactCase("c256", seed=2, children=(("ME_LN_FUSE", "0"),)),
    ExactCase("c256_d5_head8_mask10", seed=1),
    ExactCase("c512_d2_mask15", seed=2),
    ExactCase("dec512_head24_mask15", seed=1),
    ExactCase("grid16_c128_d3", seed=1, decoder=False),
    ExactCase("grid24_c64_d2", seed=3, decoder=False),
]
EXACT_BY_NAME = {c.name: c for c in EXACT}
assert len(EXACT_BY_NAME) == len(EXACT)
PAIRS = [(c.name, d) for c in EXACT for d in c.dtypes]


def _sparse_rows(rows: int, ci: int, taps: int, k: int, gen) -> torch.Tensor:
    """[rows, ci * taps] (column = channel * taps + tap) with k entries of +-1 per row, zero elsewhere.  The cells (32-channel
    slab, tap) are dealt to the rows round-robin in a shuffled order, so that every slab and every tap is hit as soon as
    rows * k reaches their number; the channel inside the slab and the sign are drawn uniformly."""
    slabs = max(1, ci // 32)
    width, cells = ci // slabs, slabs * taps
    rounds = -(-rows * k // cells)
    deal = torch.cat([torch.randperm(cells, generator=gen) for _ in range(rounds)])[:rows * k].reshape(rows, k)
    channel = (deal // taps) * width + torch.randint(0, width, (rows, k), generator=gen)
    sign = torch.randint(0, 2, (rows, k), generator=gen).float() * 2 - 1
    return torch.zeros((rows, ci * taps)).scatter_(1, channel * taps + deal % taps, sign)


def _sparse_conv(shape, k, gen):
    """[Cout, Cin, kh, kw]: k nonzeros per output channel over (cin, tap)"""
    co, ci, kh, kw = shape
    return _sparse_rows(co, ci, kh * kw, k, gen).reshape(shape)


def _sparse_convt(shape, k, gen):
    """[Cin, Cout, 2, 2]: k nonzeros per (cout, dy, dx) over cin"""
    ci, co, kh, kw = shape
    return _sparse_rows(co * kh * kw, ci, 1, k, gen).reshape(co, kh, kw, ci).permute(3, 0, 1, 2).contiguous()


def _ints(shape, bound, gen):
    """integers in [-bound, bound]"""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen).float()


def exact_checkpoint(cfg: m.ModelConfig, seed: int, nnz: Tuple[int, int] = (1, 1)) -> Dict[str, torch.Tensor]:
    """synthetic_checkpoint(cfg, seed) with the tensors of the exact paths replaced (fp16 like the rest: every value is a small
    integer).  `replaced_names` lists them."""
    w = dict(synthetic_checkpoint(cfg, seed))
    gen = torch.Generator().manual_seed(1000003 * seed + 17)
    for name, shape, kind in expected_weights(cfg):
        t = None
        if name.startswith(("decoder.", "head.", "encoder.upsample_latent0.", "encoder.upsample_latent1.")):
            k = 1
            if name.endswith(COMPOSED) and name.startswith("head."):
                k = nnz[0]
            elif name.endswith(COMPOSED) and name.startswith("decoder."):
                k = nnz[1]
            if kind == "conv":
                t = _sparse_conv(shape, k, gen)
            elif kind == "convt":
                t = _sparse_convt(shape, k, gen)
            else:                                           # bias, head_bias
                t = _ints(shape, 1, gen)
                if not (t != 0).any():
                    t[0] = 1.0                              # a short bias may draw all zeros: it would not be heard
            if name == "head.4.weight":
                t = t.abs()                                 # canonical = relu(relu(y_c) - 1): with a minus sign the closing ReLU
            elif name == "head.4.bias":                     # leaves an all-zero map, with a bias of 0 or 1 one that is zero
                t = -torch.ones(shape)                      # exactly where y_c is (or nowhere)
        elif name.startswith(COARSE_ZERO):
            t = torch.zeros(shape)                          # encodings 2 and 3 are 0 * finite, encoding 4 ...
        elif name == "encoder.fuse_lowres.bias":
            t = _ints(shape, 1, torch.Generator().manual_seed(1000003 * seed + 19))     # ... this vector at every pixel
        elif name.startswith(PATCH):
            tail = name[len(PATCH):]
            if tail == "patch_embed.proj.weight":
                t = _sparse_conv(shape, 2, gen)
            elif tail == "patch_embed.proj.bias":
                t = _ints(shape, 1, gen)
            elif tail == "cls_token":
                t = _ints(shape, 2, gen)
            elif tail == "pos_embed":
                t = _ints(shape, 1, gen)
            elif tail.endswith("attn.proj.weight"):
                t = torch.zeros(shape)                      # attention reaches the stream as 0 * finite ...
            elif tail.endswith("attn.proj.bias"):
                t = _ints(shape, 1, gen)                    # ... plus an integer vector of the block's own
            elif tail.endswith("ls1.gamma"):
                t = torch.ones(shape)
            elif tail.endswith("ls2.gamma"):
                t = torch.zeros(shape)                      # the MLP, Gaussian throughout, as 0 * finite
        if t is not None:
            w[name] = t.to(torch.float16)
    return w


def replaced_names(cfg: m.ModelConfig):
    base, new = synthetic_checkpoint(cfg, 1), exact_checkpoint(cfg, 1)
    return [n for n, _, _ in expected_weights(cfg) if not torch.equal(base[n], new[n])]


def exact_encodings(cfg: m.ModelConfig, batch: int, seed: int, scale: int = 1):
    """The five decoder inputs [B, C_i, S_i, S_i] f32 with integers in {-1, 0, 1}, different for every image of the batch.
    scale > 1 divides every spatial size (the decoder is convolutional: the sensitivity loop runs on small maps)."""
    gen = torch.Generator().manual_seed(7001 * seed + 3)
    S = cfg.img_size // scale
    chans = (cfg.dec_dim,) + tuple(cfg.enc_dims)
    return [torch.randint(-1, 2, (batch, c, S >> (i + 1), S >> (i + 1)), generator=gen, dtype=torch.int8).float()
            for i, c in enumerate(chans)]


def exact_image(cfg: m.ModelConfig, batch: int, seed: int):
    """[B, 3, S, S] f32 with values in {-1, -0.5, 0, 0.5, 1}, different for every image of the batch"""
    gen = torch.Generator().manual_seed(7013 * seed + 5)
    S = cfg.img_size
    return torch.randint(-2, 3, (batch, 3, S, S), generator=gen, dtype=torch.int8).float() * 0.5


def exact_windows(cfg: m.ModelConfig, seed: int, n: int = VIT_WINDOWS):
    """[n, 3, window, window] for the ViT entry, the values of exact_image"""
    gen = torch.Generator().manual_seed(7019 * seed + 7)
    return torch.randint(-2, 3, (n, 3, cfg.window, cfg.window), generator=gen, dtype=torch.int8).float() * 0.5


def vit_taps(cfg: m.ModelConfig):
    """the blocks tapped through the ViT entry: the model's own two, ascending (the order both sides return them in)"""
    return sorted(cfg.tap_blocks)


def inputs_of(case: ExactCase):
    cfg = case.cfg
    out = {"image": exact_image(cfg, case.batch, case.seed), "windows": exact_windows(cfg, case.seed)}
    if case.decoder:
        out["encodings"] = exact_encodings(cfg, case.batch, case.seed)
    return out


def decoder_part(w, ocfg, encodings):
    """features, lowres and -- the head on THESE features -- canonical"""
    with torch.no_grad():
        enc = [e.to(ocfg.dtype) for e in encodings]
        features, lowres = O.decoder_forward(enc, w, ocfg)
        canonical = O.head_forward(features, w, ocfg)
    return {"features": features, "lowres": lowres, "canonical": canonical}


def encoder_part(w, ocfg, image, windows, taps):
    """lat0, lat1 (encodings 0 and 1 of the whole encoder) and the tapped block outputs of the patch encoder on `windows`"""
    with torch.no_grad():
        enc = O.encoder_forward_encodings(image.to(ocfg.dtype), w, ocfg)
        _, inter = O.vit_forward_features(windows.to(ocfg.dtype), w, PATCH, ocfg, taps)
    return {"lat0": enc[0], "lat1": enc[1], "tap0": inter[0], "tap1": inter[1]}


def encoder_front(w, ocfg, image):
    """Encodings 0 and 1 alone, by the oracle's own steps (encoder.rs:238, :254-280, :307-309) on the full-resolution windows:
    what encoder_forward_encodings does for them, without the two coarser pyramid levels, the image encoder and the three other
    upsample stacks.  test_exact_cpu.py holds it equal to the whole encoder for every case, then uses it where the whole one
    would be run many times."""
    g, batch = ocfg.grid, image.shape[0]
    with torch.no_grad():
        _, taps = O.vit_forward_features(O.split(image.to(ocfg.dtype), 4, ocfg.window), w, PATCH, ocfg, list(ocfg.tap_blocks))
        lat = [O.merge(O.reshape_feature(t, g, g, 1), batch, g // 8) for t in taps]
        return {"lat0": O._upsample_block(lat[0], w, "encoder.upsample_latent0.", 3, ocfg),
                "lat1": O._upsample_block(lat[1], w, "encoder.upsample_latent1.", 2, ocfg)}


def depth_from(w, ocfg, lat0, lat1):
    """extract_depth with f_norm = 1 (mod.rs:291-362) from the two latents: encodings 2 - 4 are what COARSE_ZERO makes them"""
    b, s = lat0.shape[0], lat0.shape[2]
    e1, e2, e3 = ocfg.enc_dims[1:]
    bias = w["encoder.fuse_lowres.bias"].to(ocfg.dtype).view(1, e3, 1, 1)
    enc = [lat0, lat1, torch.zeros((b, e1, s // 4, s // 4), dtype=ocfg.dtype), torch.zeros((b, e2, s // 8, s // 8), dtype=ocfg.dtype),
           bias.expand(b, e3, s // 16, s // 16).contiguous()]
    return decoder_part(w, ocfg, enc)["canonical"].clamp(1e-4, 1e4)


def compute(case: ExactCase, w, ocfg, inputs):
    """Every compared tensor of a case from the oracle under `ocfg`, name -> tensor"""
    out = encoder_part(w, ocfg, inputs["image"], inputs["windows"], vit_taps(case.cfg))
    if case.decoder:
        out.update(decoder_part(w, ocfg, inputs["encodings"]))
    if case.e2e:
        out["depth"] = O.extract_depth(inputs["image"].to(ocfg.dtype), 1.0, w, ocfg)[0]
    return out


_REF = {}


def reference(name: str):
    """(case, weights, inputs, compared tensors of the fp32 oracle); the last case asked for is kept, so that the operand types
    and the child runs of one case share the pass"""
    if name not in _REF:
        _REF.clear()
        case = EXACT_BY_NAME[name]
        w = exact_checkpoint(case.cfg, case.seed, case.nnz)
        inputs = inputs_of(case)
        _REF[name] = (case, w, inputs, compute(case, w, oracle_cfg(case.cfg), inputs))
    return _REF[name]
