"""The configuration sweep on the GPU (-m gpu): every case of tests/config_sweep_cases.py through the HIP path, stage by stage and
end to end, against the fp32 CPU oracle on the same weights and images, at the project's own bounds (test_gpu_pipeline.py TOL and
the multipliers of test_stages_tiny / test_extract_depth_tiny).  tests/test_config_sweep_cpu.py admits each case: the reference's
own sensitivity to 16-bit operand rounding stays inside a fixed share of every bound asserted here, so a failure here is about
the kernels or their wiring.  One sweep context lives at a time; none goes into util._CTX.

Also here: every configuration me_ctx_create must refuse, each in a call of its own, with the error code validate_config names."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from matrix_eyes_amd.synthetic import synthetic_images
from oracle import depth_pro_oracle as O
from config_sweep_cases import BY_NAME, E2E_MULT, ENC_MULT, FOV_TOL_DEG, PAIRS, TOL, images_of, reference, weights_of
from util import depth_error_report, loaded_ctx, oracle_cfg, rel_l2

pytestmark = pytest.mark.gpu

ENC_NAMES = ("latent0", "latent1", "x0_features", "x1_features", "global (fuse_lowres)")
VIT_PREFIX = ("encoder.patch_encoder.", "encoder.image_encoder.", "fov.encoder.0.")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frame_and_interior(got, ref):
    """max |got - ref| / rms(ref) on the outer one-pixel frame of the last two axes and inside it"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    frame = np.ones(ref.shape[-2:], bool)
    frame[1:-1, 1:-1] = False
    scale = max(float(np.sqrt((ref ** 2).mean())), 1e-30)
    err = np.abs(got - ref)
    return float(err[..., frame].max() / scale), float(err[..., ~frame].max() / scale)


def run_stages(ctx, img, parts):
    """Every entry of the forward pass once: the stages on the ORACLE's inputs (errors do not compound), then end to end."""
    out = {}
    x = img.numpy()
    for i, e in enumerate(ctx.encoder_forward_encodings(x)):
        out[f"enc{i}"] = e
    out["features"], out["lowres"] = ctx.decoder_forward([e.numpy() for e in parts["encodings"]])
    out["canonical"] = ctx.head_forward(parts["features"].numpy())
    out["fov_stage"] = ctx.fov_forward(x, parts["lowres"].numpy())
    ctx.status_flags()
    out["depth_f1"] = ctx.extract_depth(x, 1.0)
    out["depth_fov"], out["fov_e2e"] = ctx.extract_depth(x, None, want_fov=True)
    out["flags"] = np.array(ctx.status_flags())
    return out


def check_stages(out, ref, dtype, label):
    """The assertions of test_stages_tiny / test_extract_depth_tiny on `out` (run_stages), every figure printed first."""
    w, img, inv, fov, parts = ref
    tol = TOL[dtype]
    fig = {}
    for i, (name, r) in enumerate(zip(ENC_NAMES, parts["encodings"])):
        got = out[f"enc{i}"]
        assert got.shape == tuple(r.shape), f"{label}: encoding {i} ({name}) has shape {got.shape}, the oracle's {tuple(r.shape)}"
        fr, inner = frame_and_interior(got, r.numpy())
        fig[f"enc{i}"] = (rel_l2(got, r), fr, inner)
    fig["features"] = rel_l2(out["features"], parts["features"])
    fig["lowres"] = rel_l2(out["lowres"], parts["lowres"])
    fig["canonical"] = rel_l2(out["canonical"], parts["canonical"])
    fig["canonical_frame"] = frame_and_interior(out["canonical"], parts["canonical"].numpy())
    fig["fov_stage"] = float(np.abs(out["fov_stage"] - fov.numpy()).max())
    fig["fov_e2e"] = float(np.abs(out["fov_e2e"] - fov.numpy()).max())
    inv_f1 = parts["canonical"].clamp(1e-4, 1e4).numpy()          # mod.rs:361-362 with f_norm = 1
    rep_f1 = depth_error_report(out["depth_f1"], inv_f1)
    rep_fov = depth_error_report(out["depth_fov"], inv.numpy())
    fig["depth_f1"], fig["depth_fov"] = rep_f1["rel_l2"], rep_fov["rel_l2"]
    print("sweep", label, dtype, "figures", fig)
    print("sweep", label, dtype, "depth_error_report f_norm=1", rep_f1)
    print("sweep", label, dtype, "depth_error_report fov head", rep_fov)
    for i, name in enumerate(ENC_NAMES):
        err, fr, inner = fig[f"enc{i}"]
        assert err < ENC_MULT * tol, f"{label}: encoding {i} ({name}) rel-L2 {err:.3g}"
        assert fr < 3 * inner + 1e-3, f"{label}: encoding {i} ({name}) frame {fr:.3g} against interior {inner:.3g}"
    assert fig["features"] < tol, f"{label}: features rel-L2 {fig['features']:.3g}"
    assert fig["lowres"] < tol, f"{label}: lowres rel-L2 {fig['lowres']:.3g}"
    assert np.isfinite(out["canonical"]).all(), f"{label}: canonical inverse depth is not finite"
    assert fig["canonical"] < tol, f"{label}: canonical rel-L2 {fig['canonical']:.3g}"
    fr, inner = fig["canonical_frame"]
    assert fr < 3 * inner + 1e-3, f"{label}: canonical frame {fr:.3g} against interior {inner:.3g}"
    assert fig["fov_stage"] < FOV_TOL_DEG[dtype], f"{label}: fov stage {fig['fov_stage']:.3g} deg"
    for key in ("depth_f1", "depth_fov"):
        d = out[key]
        assert np.isfinite(d).all() and d.min() >= 1e-4 and d.max() <= 1e4, f"{label}: {key} leaves the clamp of mod.rs:362"
        assert fig[key] < E2E_MULT * tol, f"{label}: {key} rel-L2 {fig[key]:.3g}"
    assert fig["fov_e2e"] < FOV_TOL_DEG[dtype], f"{label}: fov end to end {fig['fov_e2e']:.3g} deg"
    assert int(out["flags"]) == 0, f"{label}: status flags {int(out['flags'])}"
    return fig


_CHILD = """
import sys
import numpy as np, torch
root, name, dtype, mode, inputs, result = sys.argv[1:7]
sys.path.insert(0, root)
sys.path.insert(0, root + "/tests")
import matrix_eyes_amd as m
from config_sweep_cases import BY_NAME, weights_of
import test_gpu_config_sweep as T
case = BY_NAME[name]
z = np.load(inputs)
w = weights_of(case)
out = {}
if mode == "stages":
    ctx = m.Context(0, dtype, case.cfg)
    ctx.load_state_dict(w)
    parts = {"encodings": [torch.from_numpy(z[f"enc{i}"]) for i in range(5)], "features": torch.from_numpy(z["features"]),
             "lowres": torch.from_numpy(z["lowres"])}
    out = T.run_stages(ctx, torch.from_numpy(z["img"]), parts)
    out["ln_state"] = np.array(ctx.ln_fusion_state(), np.int64)
    ctx.close()
else:
    # the head from two fresh contexts; the second one's arena is filled with 0xff bytes (an f32 NaN pattern) BEFORE its weights
    # are loaded: whatever the loader does not write -- the bytes behind a short slot -- is then not finite
    for tag, poison in (("plain", False), ("poisoned", True)):
        ctx = m.Context(0, dtype, case.cfg)
        if poison:
            ctx.weight_arena_tensor().fill_(255)
            torch.cuda.synchronize()
        ctx.load_state_dict(w)
        out["canonical_" + tag] = ctx.head_forward(z["features"])
        out["depth_" + tag] = ctx.extract_depth(z["img"], 1.0)
        ctx.close()
np.savez(result, **out)
"""


def run_child(tmp_path, name, dtype, mode, ref, env=None):
    w, img, inv, fov, parts = ref
    inputs, result = str(tmp_path / f"{mode}_in.npz"), str(tmp_path / f"{mode}_out.npz")
    arrays = {"img": img.numpy(), "features": parts["features"].numpy(), "lowres": parts["lowres"].numpy()}
    if mode == "stages":
        arrays.update({f"enc{i}": e.numpy() for i, e in enumerate(parts["encodings"])})
    np.savez(inputs, **arrays)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, dtype, mode, inputs, result], env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(result)
    return {k: z[k] for k in z.files}


def check_vit_entry(ctx, case, dtype, w):
    """me_vit_forward_features for each of the three ViTs, five windows (not the 3 of the tiny test), taps on the first and the last
    block"""
    cfg = case.cfg
    xs = O.preprocess_u8(synthetic_images(5, cfg.window, case.family, seed=case.img_seed + 1))
    taps = [0, cfg.depth - 1]
    for which, prefix in enumerate(VIT_PREFIX):
        final, inter = ctx.vit_forward_features(which, xs.numpy(), taps)
        rf, ri = O.vit_forward_features(xs, w, prefix, oracle_cfg(cfg), taps)
        errs = (rel_l2(final, rf), rel_l2(inter[0], ri[0]), rel_l2(inter[1], ri[1]))
        print("sweep", case.name, dtype, "vit", which, prefix, "final / first tap / last tap rel-L2", errs)
        assert final.shape == tuple(rf.shape)
        assert max(errs) < TOL[dtype], f"{case.name}: vit {which} ({prefix}) final / taps rel-L2 {errs}"


def check_batch(ctx, case):
    """test_batch_equals_loop_of_batch_one at this configuration: a per-image stride taken from the wrong dimension shows here"""
    rgb = images_of(case)
    B = case.batch
    f_norm = np.linspace(0.8, 1.3, B).astype(np.float32)
    batch = ctx.extract_depth(rgb, f_norm)
    again = ctx.extract_depth(rgb, f_norm)
    assert np.array_equal(batch, again), f"{case.name}: a second call of the same batch differs"
    both, fovs = ctx.extract_depth(rgb, None, want_fov=True)
    both2, fovs2 = ctx.extract_depth(rgb, None, want_fov=True)
    assert np.array_equal(both, both2) and np.array_equal(fovs, fovs2), f"{case.name}: a second call (fov head) differs"
    for i in range(B):
        one = ctx.extract_depth(rgb[i:i + 1], float(f_norm[i]))
        assert np.array_equal(batch[i], one[0]), f"{case.name}: image {i} of the batch differs from its batch-one call"
        one, fov1 = ctx.extract_depth(rgb[i:i + 1], None, want_fov=True)
        assert np.array_equal(both[i], one[0]) and fovs[i] == fov1[0], f"{case.name}: image {i} (fov head) differs from batch one"
    assert len({batch[i].tobytes() for i in range(B)}) == B


@pytest.mark.parametrize("name,dtype", PAIRS, ids=[f"{n}-{d}" for n, d in PAIRS])
def test_case_against_the_oracle(name, dtype, tmp_path):
    case = BY_NAME[name]
    cfg = case.cfg
    ref = reference(name)
    w, img, inv, fov, parts = ref
    ctx = m.Context(0, dtype, cfg)
    try:
        ctx.load_state_dict(w)
        out = run_stages(ctx, img, parts)
        ln_state = ctx.ln_fusion_state()
        check_stages(out, ref, dtype, name)
        if cfg.embed_dim >= 256:
            # the residual launches carry the LayerNorm (C in {256, 512, 1024}) and no step was run again without it
            print("sweep", name, dtype, "ln_fusion_state (fused, fallbacks)", ln_state)
            assert ln_state == (True, 0), f"{name}: LayerNorm fusion state {ln_state}"
        if case.batch > 1:
            check_batch(ctx, case)
        if case.vit_entry:
            check_vit_entry(ctx, case, dtype, w)
    finally:
        ctx.close()
    if cfg.head_dims[0] < 32:
        # EPI_HEAD_COMPOSED multiplies 32 channels whatever head_dims[0] is; head.4.weight holds head_dims[0] floats.  What lies
        # behind it in one process says nothing: two fresh contexts in a child, one over an arena of NaN patterns
        z = run_child(tmp_path, name, dtype, "head", ref)
        for tag in ("plain", "poisoned"):
            canon = z["canonical_" + tag]
            assert np.isfinite(canon).all() and np.isfinite(z["depth_" + tag]).all(), f"{name}: head output not finite ({tag} arena)"
            assert rel_l2(canon, parts["canonical"]) < TOL[dtype], f"{name}: canonical ({tag} arena)"
            assert np.array_equal(canon, out["canonical"]), f"{name}: the head of a fresh context ({tag} arena) differs from this one's"
            assert np.array_equal(z["depth_" + tag], out["depth_f1"]), f"{name}: depth of a fresh context ({tag} arena) differs"
    if case.ln_unfused_child and dtype == "f16":
        # the same case on the stand-alone LayerNorm launches (ME_LN_FUSE=0), held to the oracle at the same bounds
        z = run_child(tmp_path, name, dtype, "stages", ref, env={"ME_LN_FUSE": "0"})
        check_stages(z, ref, dtype, name + " ME_LN_FUSE=0")
        differs = not np.array_equal(z["depth_fov"], out["depth_fov"])
        print("sweep", name, "fused LayerNorm against ME_LN_FUSE=0: rel-L2", rel_l2(out["depth_fov"], z["depth_fov"]),
              "" if differs else "-- IDENTICAL: the residency query declined the fused route on this device, both runs are the "
              "stand-alone launches")
        assert tuple(z["ln_state"]) == (1, 0)


def _bad(**kw):
    base = m.ModelConfig.tiny().__dict__
    return m.ModelConfig(**{**base, **kw})


# (what, configuration, error code validate_config names: 2 = ME_ERR_BAD_SHAPE, 1 = ME_ERR_BAD_ARG)
REJECTED = [
    ("grid 0", _bad(grid=0), 2), ("grid 12", _bad(grid=12), 2), ("grid 72", _bad(grid=72), 2),
    ("embed_dim 192, 3 heads", _bad(embed_dim=192, num_heads=3), 2), ("embed_dim 128, 3 heads", _bad(embed_dim=128, num_heads=3), 2),
    ("depth 0", _bad(depth=0, tap_blocks=(0, 1)), 2), ("depth 65", _bad(depth=65), 2),
    ("taps equal", _bad(tap_blocks=(2, 2)), 2), ("tap = depth", _bad(tap_blocks=(1, 4)), 2), ("negative tap", _bad(tap_blocks=(-1, 2)), 2),
    ("enc_dims entry 0", _bad(enc_dims=(64, 0, 128, 128)), 2), ("enc_dims entry 96", _bad(enc_dims=(64, 128, 96, 128)), 2),
    ("dec_dim 128", _bad(dec_dim=128), 2), ("dec_dim 384", _bad(dec_dim=384), 2),
    ("head_dims (36,1)", _bad(head_dims=(36, 1)), 2), ("head_dims (6,1)", _bad(head_dims=(6, 1)), 2),
    ("head_dims (32,2)", _bad(head_dims=(32, 2)), 2),
    ("ln_eps 0", _bad(ln_eps=0.0), 1),
    ("split_operands -1", _bad(split_operands=-1), 1), ("split_operands 16", _bad(split_operands=16), 1),
]


def test_rejected_configurations_then_a_good_one():
    """validate_config's messages are the specification: each refused value in a me_ctx_create call of its own, with the code it
    names and a message; afterwards a tiny context is created, loaded and run as if nothing had happened."""
    for what, cfg, code in REJECTED:
        with pytest.raises(m.MatrixEyesError) as e:
            m.Context(0, "f16", cfg)
        assert e.value.code == code, f"{what}: code {e.value.code}, message {e.value.message!r}"
        assert e.value.message.strip(), what
    assert len({what for what, _, _ in REJECTED}) == len(REJECTED) == 20
    tiny = BY_NAME["tiny"]
    rgb = images_of(tiny)
    want, want_fov = loaded_ctx("tiny", "f16").extract_depth(rgb, None, want_fov=True)
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    try:
        ctx.load_state_dict(weights_of(tiny))
        got, got_fov = ctx.extract_depth(rgb, None, want_fov=True)
    finally:
        ctx.close()
    assert np.array_equal(got, want) and np.array_equal(got_fov, want_fov)
