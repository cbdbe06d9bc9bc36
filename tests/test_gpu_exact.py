"""Exact-arithmetic checkpoints on the GPU (-m gpu): the conv stages and the ViT taps of the HIP path held to the fp32 CPU oracle
BIT FOR BIT.  tests/exact_cases.py builds checkpoints and inputs of small integers for which every operand, product, partial sum
and intermediate is exactly representable; tests/test_exact_cpu.py shows from the reference alone that f32, f64, f16 operands
and bf16 operands then give the same bits, that the maps are not trivial and that every layer is heard.  So nothing here is
rounding: operand types, the order of the f32 sums, hi + lo operands, the load-time compositions (weights.hip compose_head,
compose_features, out_conv o deconv) and GemmParams::tap_bias must all leave the integers alone, and an indexing, phase, stride,
tap-routing or border-share error is a whole-integer difference.  Every assertion is array equality.

Entries: decoder_forward(exact encodings) -> features, lowres; head_forward(the oracle's features) -> canonical;
encoder_forward_encodings(exact image) -> encodings 0 and 1 (2-4 pass the final LayerNorm and the bilinear pyramid: not exact,
not compared); vit_forward_features(patch encoder, exact windows) -> the tapped block outputs; and, on the cases marked e2e,
extract_depth(exact image, f_norm = 1) -> depth.  Which entry runs which composition: head_forward runs compose_head;
decoder_forward runs out_conv o deconv but hands out the f32 feature map, so it keeps out_conv and head[0] apart, and
head_forward takes that map -- compose_features and tap_bias run in extract_depth ALONE, which is why it is here (exact_cases.py
COARSE_ZERO makes it exact).  ME_FEAT_COMPOSED=0 therefore changes the launches of that entry only.  The switches the library reads
once per process (ME_HEAD_COMPOSED, ME_FEAT_COMPOSED, ME_LN_FUSE) run in child processes, one after another: both routes equal the
oracle, hence each other.  One context lives at a time; none goes into util._CTX."""
import os
import subprocess
import sys

import numpy as np
import pytest

import matrix_eyes_amd as m
import exact_cases as X
from exact_cases import EXACT_BY_NAME, PAIRS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the compared arrays that are maps ([B, C, H, W], canonical [B, H, W]); the tapped blocks are [window, token, channel]
MAPS = ("features", "lowres", "canonical", "lat0", "lat1", "depth")
BATCH_LOOP_CASE = "tiny_head16"


def difference(key, got, ref):
    """'' when the arrays are equal; otherwise where the first differing element is -- by channel, pixel and whether it lies on
    the one-pixel frame of its map -- and how many elements differ on the frame and inside it.  That report is the diagnosis."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"{key}: shape {got.shape}, the oracle's {ref.shape}"
    if np.array_equal(got, ref):
        return ""
    bad = got != ref
    first = tuple(int(i) for i in np.argwhere(bad)[0])
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    msg = f"{key}: {int(bad.sum())} of {bad.size} elements differ, largest |difference| {np.nanmax(d):g}, finite {bool(np.isfinite(got).all())}; first at "
    if key in MAPS:
        frame = np.ones(ref.shape[-2:], bool)
        frame[1:-1, 1:-1] = False
        y, x = first[-2:]
        where = f"image {first[0]}, " + (f"channel {first[1]}, " if got.ndim == 4 else "") + f"pixel (y {y}, x {x})"
        msg += (f"{where}, {'ON' if frame[y, x] else 'inside'} the one-pixel frame: got {got[first]:g}, the oracle {ref[first]:g}; "
                f"{int(bad[..., frame].sum())} differ on the frame, {int(bad[..., ~frame].sum())} inside; "
                f"images that differ {sorted(set(np.argwhere(bad)[:, 0].tolist()))}")
        if got.ndim == 4:
            msg += f", channels that differ {int(bad.any(axis=(0, 2, 3)).sum())} of {got.shape[1]}"
    else:       # a tapped block [window, token, channel]
        msg += (f"window {first[0]}, token {first[1]} ({'the class token' if first[1] == 0 else 'a patch'}), channel {first[2]}: "
                f"got {got[first]:g}, the oracle {ref[first]:g}; tokens that differ {int(bad.any(axis=(0, 2)).sum())} of {got.shape[1]}")
    return msg


def run_entries(ctx, case, inputs, features):
    """Every exact entry once, name -> array; me_status_flags has to read 0 after each call (nothing overflows at these
    magnitudes).  `features`: the ORACLE's feature map, so that the head is judged on its own."""
    out, flags = {}, []
    if case.decoder:
        out["features"], out["lowres"] = ctx.decoder_forward([e.numpy() for e in inputs["encodings"]])
        flags.append(("decoder_forward", ctx.status_flags()))
        out["canonical"] = ctx.head_forward(features)
        flags.append(("head_forward", ctx.status_flags()))
    enc = ctx.encoder_forward_encodings(inputs["image"].numpy())
    flags.append(("encoder_forward_encodings", ctx.status_flags()))
    out["lat0"], out["lat1"] = enc[0], enc[1]
    _, inter = ctx.vit_forward_features(0, inputs["windows"].numpy(), X.vit_taps(case.cfg))
    flags.append(("vit_forward_features", ctx.status_flags()))
    out["tap0"], out["tap1"] = inter
    if case.e2e:
        # the one entry whose decoder leaves out_conv to the head: compose_features and GemmParams::tap_bias run here only
        out["depth"] = ctx.extract_depth(inputs["image"].numpy(), 1.0)
        flags.append(("extract_depth", ctx.status_flags()))
    out["flags"] = np.array([f for _, f in flags], np.int64)
    assert all(f == 0 for _, f in flags), f"{case.name}: status flags {flags}"
    return out


def check(out, ref, label):
    report = [difference(key, out[key], r.numpy()) for key, r in ref.items()]
    report = [r for r in report if r]
    assert not report, f"{label}: the HIP path differs from the fp32 oracle\n" + "\n".join(report)
    assert not out["flags"].any(), f"{label}: status flags {out['flags']}"


_CHILD = """
import sys
import numpy as np, torch
root, name, dtype, mode, features, result = sys.argv[1:7]
sys.path.insert(0, root)
sys.path.insert(0, root + "/tests")
import matrix_eyes_amd as m
import exact_cases as X
import test_gpu_exact as T
case = X.EXACT_BY_NAME[name]
w, inputs = X.exact_checkpoint(case.cfg, case.seed, case.nnz), X.inputs_of(case)
ctx = m.Context(0, dtype, case.cfg)
if mode == "poisoned":
    # the arena filled with 0xff bytes (an f32 NaN pattern) BEFORE the weights are loaded: whatever the loader does not write is
    # then not finite, and no integer
    ctx.weight_arena_tensor().fill_(255)
    torch.cuda.synchronize()
ctx.load_state_dict(w)
out = T.run_entries(ctx, case, inputs, np.load(features))
out["ln_state"] = np.array(ctx.ln_fusion_state(), np.int64)
ctx.close()
np.savez(result, **out)
"""


def run_child(tmp_path, name, dtype, mode, ref, env):
    feat, result = str(tmp_path / "features.npy"), str(tmp_path / f"{mode}_out.npz")
    np.save(feat, ref["features"].numpy() if "features" in ref else np.zeros(1, np.float32))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, dtype, mode, feat, result], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name} {mode} {env}: exit status {r.returncode}\n" + r.stderr[-3000:]
    z = np.load(result)
    return {k: z[k] for k in z.files}


def check_batch(ctx, case, inputs, ref, out):
    """A batch is a loop of batch-one calls.  That follows from equality with the oracle; asserted anyway, entry by entry."""
    for i in range(case.batch):
        feat, low = ctx.decoder_forward([e[i:i + 1].numpy() for e in inputs["encodings"]])
        canon = ctx.head_forward(ref["features"][i:i + 1].numpy())
        enc = ctx.encoder_forward_encodings(inputs["image"][i:i + 1].numpy())
        depth = ctx.extract_depth(inputs["image"][i:i + 1].numpy(), 1.0)
        one = {"features": feat, "lowres": low, "canonical": canon, "lat0": enc[0], "lat1": enc[1], "depth": depth}
        for key, a in one.items():
            assert np.array_equal(a[0], out[key][i]), f"{case.name}: {key} of image {i} alone differs from its place in the batch"
    assert ctx.status_flags() == 0


@pytest.mark.parametrize("name,dtype", PAIRS, ids=[f"{n}-{d}" for n, d in PAIRS])
def test_case_equals_the_oracle(name, dtype, tmp_path):
    case, w, inputs, ref = X.reference(name)
    cfg = case.cfg
    features = ref["features"].numpy() if case.decoder else None
    ctx = m.Context(0, dtype, cfg)
    try:
        ctx.load_state_dict(w)
        out = run_entries(ctx, case, inputs, features)
        ln_state = ctx.ln_fusion_state()
        check(out, ref, f"{name} [{dtype}]")
        if cfg.embed_dim >= 256:
            # the residual launches of this case carry the LayerNorm, and no step was run again without it
            assert ln_state == (True, 0), f"{name}: LayerNorm fusion state {ln_state}"
        if name == BATCH_LOOP_CASE:
            assert case.batch > 1
            check_batch(ctx, case, inputs, ref, out)
    finally:
        ctx.close()
    if dtype != case.dtypes[0]:
        return
    # the switches read once per process, each in a fresh child, one after another
    for var, value in case.children:
        z = run_child(tmp_path, name, dtype, "plain", ref, {var: value})
        check(z, ref, f"{name} [{dtype}] {var}={value}")
        if var == "ME_LN_FUSE":
            assert tuple(z["ln_state"]) == (1, 0)           # no step fell back (the state is about fall-backs, not the switch)
    if name == BATCH_LOOP_CASE:
        z = run_child(tmp_path, name, dtype, "poisoned", ref, {})
        check(z, ref, f"{name} [{dtype}] over a poisoned arena")
