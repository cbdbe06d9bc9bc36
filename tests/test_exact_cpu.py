"""The exact-arithmetic checkpoints, CPU side (no GPU): every case of tests/exact_cases.py is ADMITTED from the reference alone.

(a) Exactness: the oracle gives the same bits in f32, in f64 and with both operands of every linear / convolution call rounded to
    f16 or to bf16, and nothing larger than the type's integer range enters such a call.  These are conditions, not
    measurements: a case that fails gets another seed or fewer nonzeros, never a tolerance.
(b) Non-triviality: every compared tensor takes many values and is neither mostly zero nor never zero.
(c) Support coverage: over the table, every 3x3 tap, every ConvTranspose phase and every 32-channel slab of every input width
    carries a nonzero weight, and every bias has nonzero entries.
(d) Sensitivity (tiny): zeroing any replaced tensor, rolling any 3x3 weight by a tap, exchanging the phases of any
    ConvTranspose and exchanging the two taps each change a compared tensor -- the checkpoint listens to every layer, so an error
    of the HIP path in that layer cannot cancel.

tests/test_gpu_exact.py then holds the HIP path EQUAL to the fp32 oracle on the same cases."""
import pytest
import torch

from matrix_eyes_amd.config import expected_weights
from oracle import depth_pro_oracle as O
import exact_cases as X
from exact_cases import EXACT, EXACT_BY_NAME, PATCH
from util import oracle_cfg

NAMES = [c.name for c in EXACT]
# lowres is ONE sparse convolution (decoder.convs.4: a single +-1 per row, no bias) of a map over {-1, 0, 1}: three values are
# all it can take, and it has to take all three
MANY, FEW = 16, {"lowres": 3}


def _modes(cfg):
    f32, f64, h, b = (oracle_cfg(cfg) for _ in range(4))
    f64.dtype = torch.float64
    h.operand_dtype, b.operand_dtype = torch.float16, torch.bfloat16
    return {"f32": f32, "f64": f64, "f16 operands": h, "bf16 operands": b}


class Magnitude:
    """O._ops wrapped: the largest |value| of either operand over every linear / convolution call"""

    def __init__(self, monkeypatch):
        self.max, self.calls = 0.0, 0
        self.take()
        inner = O._ops

        def ops(cfg, x, w):
            self.max = max(self.max, float(x.abs().max()), float(w.abs().max()))
            self.calls += 1
            return inner(cfg, x, w)
        monkeypatch.setattr(O, "_ops", ops)

    def take(self):
        """the largest operand since the last take"""
        got, self.max = getattr(self, "max", 0.0), 0.0
        return got


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.to(torch.float64), b.to(torch.float64))


@pytest.mark.parametrize("name", NAMES)
def test_case_is_exact_and_not_trivial(name, monkeypatch):
    case = EXACT_BY_NAME[name]
    cfg, taps = case.cfg, X.vit_taps(case.cfg)
    w, inputs, modes = X.exact_checkpoint(cfg, case.seed, case.nnz), X.inputs_of(case), _modes(cfg)
    # What the GPU file compares with -- the whole batch, the whole encoder, fp32 (X.compute, part by part) -- with every operand
    # measured.  The decoder entry runs on integers; the encoder and the end-to-end pass on halves (the image is in halves), which
    # 16-bit operands hold exactly up to half the limit only
    mag = Magnitude(monkeypatch)
    ref = X.encoder_part(w, modes["f32"], inputs["image"], inputs["windows"], taps)
    largest = {"encoder": (mag.take(), case.limit / 2)}
    if case.decoder:
        ref.update(X.decoder_part(w, modes["f32"], inputs["encodings"]))
        largest["decoder"] = (mag.take(), case.limit)
    if case.e2e:
        ref["depth"] = O.extract_depth(inputs["image"], 1.0, w, modes["f32"])[0]
        largest["end to end"] = (mag.take(), case.limit / 2)
    # The other three modes on the first image (the windows of the ViT entry in full).  For the other images the magnitudes just
    # measured say the same: values below those limits are exact operands in all three, and sums of their products with +-1 are
    # exact in f32 as in f64.  The first two encodings come by encoder_front, the depth by depth_from, held equal to the whole
    # encoder and to extract_depth here
    one = {k: ([e[:1] for e in v] if k == "encodings" else v[:1] if k == "image" else v) for k, v in inputs.items()}
    for mode in ("f32", "f64", "f16 operands", "bf16 operands"):
        ocfg = modes[mode]
        if mode == "f32":
            got = X.encoder_front(w, ocfg, inputs["image"])
            if case.e2e:
                got["depth"] = X.depth_from(w, ocfg, got["lat0"], got["lat1"])
            assert all(torch.equal(g, ref[key]) for key, g in got.items())
            continue
        got = X.encoder_front(w, ocfg, one["image"])
        if True:
            with torch.no_grad():
                _, inter = O.vit_forward_features(inputs["windows"].to(ocfg.dtype), w, PATCH, ocfg, taps)
            if case.e2e:
                got["depth"] = X.depth_from(w, ocfg, got["lat0"], got["lat1"])
            got.update(tap0=inter[0], tap1=inter[1])
            if case.decoder:
                got.update(X.decoder_part(w, ocfg, one["encodings"]))
            assert set(got) == set(ref)
        for key, g in got.items():
            r = ref[key] if key in ("tap0", "tap1") else ref[key][:1]
            if key == "depth":
                g = g.to(torch.float32)     # the clamp's floor 1e-4 is the one value here that f32 and f64 hold differently
            assert _same(g, r), f"{name}: {key} of the oracle with {mode} differs from the fp32 oracle: re-seed or thin the case"
    print("exact", name, "largest operand, limit:", largest, "over", mag.calls, "calls")
    assert mag.calls > 0
    for part, (top, limit) in largest.items():
        assert 0 < top <= limit, f"{name}: |operand| of the {part} part reaches {top}, past {limit}"
    for key, r in ref.items():
        zero = 1e-4 if key == "depth" else 0.0              # the clamp of mod.rs:362 puts the zeros of the closing ReLU there
        distinct, nonzero, top = int(r.unique().numel()), float((r > zero).float().mean() if zero else (r != 0).float().mean()), float(r.abs().max())
        print("exact", name, key, tuple(r.shape), "distinct", distinct, "nonzero %.3f" % nonzero, "max", top)
        assert torch.isfinite(r).all() and top <= case.limit
        assert distinct >= MANY or distinct == FEW.get(key), f"{name}: {key} takes {distinct} values"
        assert 0.10 <= nonzero <= 0.95, f"{name}: {nonzero:.1%} of {key} is nonzero"
    assert not torch.equal(ref["tap0"], ref["tap1"]), f"{name}: the two tapped blocks give the same output"
    if case.batch > 1:
        for key, r in ref.items():
            if key not in ("tap0", "tap1"):
                assert not torch.equal(r[0], r[1]), f"{name}: {key} is the same for two images of the batch"


def _layers():
    """(case, name, kind, tensor) of every replaced weight of every case"""
    for case in EXACT:
        w = X.exact_checkpoint(case.cfg, case.seed, case.nnz)
        replaced = set(X.replaced_names(case.cfg))
        for name, shape, kind in expected_weights(case.cfg):
            if name in replaced:
                yield case, name, kind, w[name].float()


def test_support_coverage():
    """Counted over the table: a layer is covered when some case's checkpoint puts a nonzero there.  (One checkpoint cannot: the
    head.2 of a 4-channel head has eight nonzeros for nine taps.)  Slabs are counted per input width, since cases with other
    widths have other slabs."""
    taps, phases, slabs, biases = {}, {}, {}, {}
    for case, name, kind, t in _layers():
        if name.endswith(("attn.proj.weight", "gamma", "cls_token", "pos_embed")) or name.startswith(X.COARSE_ZERO):
            continue
        if kind == "conv":
            co, ci, kh, kw = t.shape
            if (kh, kw) == (3, 3):
                taps[name] = taps.get(name, torch.zeros(9, dtype=torch.bool)) | (t != 0).reshape(co * ci, 9).any(0)
            if ci % 32 == 0:
                hit = (t != 0).reshape(co, ci // 32, 32 * kh * kw).any(2).any(0)
                slabs[(name, ci)] = slabs.get((name, ci), torch.zeros(ci // 32, dtype=torch.bool)) | hit
        elif kind == "convt":
            ci, co, kh, kw = t.shape
            phases[name] = phases.get(name, torch.zeros(4, dtype=torch.bool)) | (t != 0).reshape(ci * co, 4).any(0)
            hit = (t != 0).reshape(ci // 32, 32 * co * 4).any(1)
            slabs[(name, ci)] = slabs.get((name, ci), torch.zeros(ci // 32, dtype=torch.bool)) | hit
        else:
            biases[(case.name, name)] = bool((t != 0).any())
    assert len(taps) >= 4 + 20 + 2 and len(phases) == 4 + 1 + 5 and len(biases) > 20 * len(EXACT)
    assert all(v.all() for v in taps.values()), [k for k, v in taps.items() if not v.all()]
    assert all(v.all() for v in phases.values()), [k for k, v in phases.items() if not v.all()]
    assert all(v.all() for v in slabs.values()), [k for k, v in slabs.items() if not v.all()]
    assert all(biases.values()), [k for k, v in biases.items() if not v]


# --- sensitivity, tiny --------------------------------------------------------------------------------------------------------
SCALE = 4       # the decoder and the head are convolutions: the loop runs them on maps a quarter of the size, batch one


def _sensitivity_setup():
    case = EXACT_BY_NAME["tiny"]
    cfg = case.cfg
    w = X.exact_checkpoint(cfg, case.seed, case.nnz)
    ocfg = oracle_cfg(cfg)
    enc = X.exact_encodings(cfg, 1, case.seed, SCALE)
    image = X.exact_image(cfg, 1, case.seed)
    return case, cfg, w, ocfg, enc, image


def _front(w, ocfg, image, windows):
    """the first two encodings, and the tapped blocks through the ViT entry (which alone keep the class token)"""
    out = X.encoder_front(w, ocfg, image)
    with torch.no_grad():
        _, inter = O.vit_forward_features(windows, w, PATCH, ocfg, X.vit_taps(ocfg))
    out.update(tap0=inter[0], tap1=inter[1])
    # end to end from a corner of the two latents (fuse_lowres.bias is heard nowhere else)
    out["depth"] = X.depth_from(w, ocfg, out["lat0"][:, :, :64, :64], out["lat1"][:, :, :32, :32])
    return out


def _changed(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a)


def test_every_layer_is_heard():
    case, cfg, w, ocfg, enc, image = _sensitivity_setup()
    windows = X.exact_windows(cfg, case.seed, 1)
    base_dec, base_enc = X.decoder_part(w, ocfg, enc), _front(w, ocfg, image, windows)
    assert int(base_dec["canonical"].unique().numel()) >= MANY         # the small maps are still a live experiment
    last_tap = max(cfg.tap_blocks)
    shapes = {n: (s, k) for n, s, k in expected_weights(cfg)}

    def run(name, t):
        mutated = dict(w)
        mutated[name] = t.to(torch.float16)
        if name.startswith("encoder."):
            return _changed(_front(mutated, ocfg, image, windows), base_enc)
        return _changed(X.decoder_part(mutated, ocfg, enc), base_dec)

    zeroed = rolled = swapped = 0
    for name in X.replaced_names(cfg):
        t = w[name].float()
        if name.startswith(PATCH + "blocks."):
            if int(name[len(PATCH + "blocks."):].split(".")[0]) > last_tap:
                continue                    # behind the last tap: it reaches encodings 2-4 only, which are not compared
        if not (t != 0).any():
            continue                        # attn.proj.weight, ls2.gamma, the coarse upsample stacks, fuse_lowres.weight: zero by construction
        if name.startswith("decoder.fusions.4.resnet1."):
            continue                        # the deepest fusion block has one input: its first residual unit is never run (decoder.rs:179)
        assert run(name, torch.zeros_like(t)), f"zeroing {name} changes nothing"
        zeroed += 1
        kind = shapes[name][1]
        if kind == "conv" and tuple(t.shape[2:]) == (3, 3):
            assert run(name, t.reshape(t.shape[0], t.shape[1], 9).roll(1, 2).reshape(t.shape)), f"rolling {name} by a tap changes nothing"
            rolled += 1
        if kind == "convt":
            assert run(name, t.transpose(2, 3)), f"exchanging the phases (0,1) and (1,0) of {name} changes nothing"
            assert run(name, t.flip(2)), f"exchanging the rows dy = 0, 1 of {name} changes nothing"
            swapped += 1
    print("sensitivity: zeroed", zeroed, "rolled", rolled, "phase-swapped", swapped)
    assert rolled == 4 + 18 + 2 and swapped == 4 + 1 + 5 and zeroed >= 75


def test_the_two_taps_are_told_apart(monkeypatch):
    """OracleConfig.tap_blocks is a set to the oracle (vit.rs:297-326 collects blocks in ascending order), so exchanging its
    entries changes nothing there; what a HIP path could get wrong is which tapped block feeds which upsample stack.  That
    exchange, made in the oracle, changes both latents."""
    case, cfg, w, ocfg, enc, image = _sensitivity_setup()
    base = X.encoder_front(w, ocfg, image)
    inner = O.vit_forward_features

    def exchanged(xs, weights, p, c, intermediate_blocks=()):
        final, taps = inner(xs, weights, p, c, intermediate_blocks)
        return final, taps[::-1]
    monkeypatch.setattr(O, "vit_forward_features", exchanged)
    other = X.encoder_front(w, ocfg, image)
    assert not torch.equal(other["lat0"], base["lat0"]) and not torch.equal(other["lat1"], base["lat1"])
