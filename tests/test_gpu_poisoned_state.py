"""The question of test_gpu_redzone.py one level up (-m gpu): does a depth map depend on bytes the pipeline never wrote?

Arena gaps.  me_ctx_create zeroes the weight arena, so the alignment gap behind every weight slot is finite in every other
test.  Here the whole arena is filled with 0xFF -- NaN in f16, bf16 and f32 -- before any weight is loaded, through
me_weight_arena_ptr / me_weight_arena_bytes and one hipMemset of the HIP runtime the process already has; the loaded context
must give a finite depth and FOV, bit for bit those of a context whose arena was created normally.  A read past a slot -- the
composed head once read w2[16 .. 31] behind a 16-float head.4.weight (DESIGN.md "What the tests found") -- is then 0 * NaN.
Both packers, both 16-bit types, the FOV head and a given f_norm; the tiny configuration and the sweep's head_dims[0] = 16 one,
the shape of that defect.  An ME_DTYPE_FP8 context's second arena (the e4m3 copies of the ViT weights) has no exposed pointer:
it is left out here.

History.  The site buffers are zeroed once and then reused with whatever the step before left in them.  One loaded context
computes extract_depth(A), then runs other images (one of them noise at ten times the amplitude), fov_forward, head_forward
and decoder_forward on unrelated data and a step with f_norm given, and computes extract_depth(A) again: the same bits, and
those of a fresh context; once more with the captured graph (eager, capture, replay)."""
import ctypes as C

import numpy as np
import pytest
import torch

import config_sweep_cases as SW
import matrix_eyes_amd as m
from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images

pytestmark = pytest.mark.gpu


def _hip():
    """the HIP runtime library torch loaded into this process"""
    with open("/proc/self/maps") as maps:
        for line in maps:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime is loaded")


def poison_arena(ctx):
    """0xFF over the whole weight arena"""
    hip = _hip()
    hip.hipMemset.argtypes, hip.hipMemset.restype = [C.c_void_p, C.c_int, C.c_size_t], C.c_int
    hip.hipDeviceSynchronize.argtypes, hip.hipDeviceSynchronize.restype = [], C.c_int
    ptr, n = ctx.lib.me_weight_arena_ptr(ctx.handle), ctx.weight_arena_bytes()
    assert ptr and n > 0
    ctx.synchronize()
    assert hip.hipMemset(C.c_void_p(ptr), 0xFF, n) == 0
    assert hip.hipDeviceSynchronize() == 0
    assert bool((ctx.weight_arena_tensor() == 0xFF).all())


_CFGS = {"tiny": (m.ModelConfig.tiny(), 2024), "tiny_head16": (SW.BY_NAME["tiny_head16"].cfg, SW.BY_NAME["tiny_head16"].ckpt_seed)}
assert _CFGS["tiny_head16"][0].head_dims[0] < 32
_WEIGHTS = {}


def _weights(name):
    if name not in _WEIGHTS:
        cfg, seed = _CFGS[name]
        _WEIGHTS[name] = synthetic_checkpoint(cfg, seed=seed)
    return _WEIGHTS[name]


def _loaded(name, dtype, packer, poisoned=False):
    ctx = m.Context(0, dtype, _CFGS[name][0], weight_packer=packer)
    if poisoned:
        poison_arena(ctx)
    ctx.load_state_dict(_weights(name))
    return ctx


def _run(ctx, rgb):
    ctx.status_flags()
    depth, fov = ctx.extract_depth(rgb, None, want_fov=True)
    given = ctx.extract_depth(rgb, np.array([0.8, 1.3], np.float32)[:rgb.shape[0]])
    assert ctx.status_flags() == 0
    return depth, fov, given


@pytest.mark.parametrize("packer", ["host", "device"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(_CFGS))
def test_depth_does_not_depend_on_the_arena_gaps(name, dtype, packer):
    rgb = synthetic_images(2, _CFGS[name][0].img_size, "structured", seed=5)
    clean = _loaded(name, dtype, packer)
    want = _run(clean, rgb)
    clean_arena = clean.weight_arena_tensor().cpu()
    clean.close()
    ctx = _loaded(name, dtype, packer, poisoned=True)
    arena = ctx.weight_arena_tensor().cpu()
    gaps = arena != clean_arena
    assert bool(gaps.any()) and bool((arena[gaps] == 0xFF).all()) and bool((clean_arena[gaps] == 0).all())       # there are gaps, and only gaps differ
    got = _run(ctx, rgb)
    ctx.close()
    for g, w, what in zip(got, want, ("depth", "fov", "depth with f_norm given")):
        assert np.isfinite(g).all(), what
        assert np.array_equal(g, w), what


def _history(ctx, cfg, seed):
    """steps that leave other values in every site buffer"""
    S, g = cfg.img_size, cfg.grid
    others = synthetic_images(3, S, "structured", seed=seed).astype(np.float32)
    x = (others.transpose(0, 3, 1, 2) / 255.0 - 0.5) / 0.5
    rng = np.random.default_rng(seed)
    x[1] = rng.standard_normal(x[1].shape).astype(np.float32) * 10.0            # noise at ten times the amplitude
    ctx.extract_depth(np.ascontiguousarray(x, np.float32), None)
    low = rng.standard_normal((2, cfg.dec_dim, 2 * g, 2 * g)).astype(np.float32)
    ctx.fov_forward(np.ascontiguousarray(x[:2]), low)
    ctx.head_forward(rng.standard_normal((1, cfg.dec_dim, S // 2, S // 2)).astype(np.float32) * 3.0)
    enc = [rng.standard_normal(s).astype(np.float32) * 2.0 for s in ctx._enc_shapes(2)]
    ctx.decoder_forward(enc)
    ctx.extract_depth(synthetic_images(2, S, "noise", seed=seed + 1), np.array([0.7, 1.9], np.float32))
    ctx.status_flags()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_depth_does_not_depend_on_earlier_steps(dtype):
    cfg = m.ModelConfig.tiny()
    A = synthetic_images(1, cfg.img_size, "structured", seed=11)
    fresh = _loaded("tiny", dtype, "host")
    want = fresh.extract_depth(A, None, want_fov=True)
    fresh.close()
    ctx = _loaded("tiny", dtype, "host")
    first = ctx.extract_depth(A, None, want_fov=True)
    for rnd in range(2):
        _history(ctx, cfg, 100 + rnd)
        again = ctx.extract_depth(A, None, want_fov=True)
        for a, f, w in zip(again, first, want):
            assert np.isfinite(a).all() and np.array_equal(a, f) and np.array_equal(a, w), rnd
    ctx.close()


def test_depth_does_not_depend_on_earlier_steps_under_the_graph():
    """device pointers only, so that the call is eager, then captured, then replayed: each of the three after a history of other
    steps (host-pointer calls, which run eagerly and drop nothing)"""
    cfg = m.ModelConfig.tiny()
    S = cfg.img_size
    A = torch.from_numpy(synthetic_images(1, S, "structured", seed=11)).cuda()
    fresh = _loaded("tiny", "f16", "host")
    want = fresh.extract_depth(A.cpu().numpy(), None)
    fresh.close()
    ctx = _loaded("tiny", "f16", "host")
    ctx.set_graph(True)
    rgb = A.clone()
    out = torch.empty(1, S, S, dtype=torch.float32, device="cuda")
    n0 = ctx.graph_launch_count
    for i in range(4):                                   # eager, captured and launched, replayed twice
        _history(ctx, cfg, 200 + i)
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        ctx.extract_depth(rgb, None, out=out)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), i
    assert ctx.graph_launch_count >= n0 + 2
    ctx.close()
