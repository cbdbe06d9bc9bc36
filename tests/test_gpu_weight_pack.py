"""GPU tests of the device weight packer (csrc/weight_pack.hip) and the arena cache: every pack kernel against the numpy /
torch restatement of tests/weight_pack_cases.py, exact; the whole tiny model packed on the device against the host packer's
arena byte for byte, with the depth bits; the cache file's round trip, its damaged and stale forms and the policy of
me_load_checkpoint_cached; --convert-checkpoints in both command lines."""
import ctypes as C
import dataclasses
import glob
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_pack_cases as W  # noqa: E402
from util import ctx_for, run_cli, tiny_checkpoint, weights_for  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
SRC_DTYPES = [W.W_F16, W.W_BF16, W.W_F32, W.W_F64]
ME_ERR_BAD_ARG, ME_ERR_BAD_SHAPE, ME_ERR_IO, ME_ERR_NOT_READY = 1, 2, 7, 8
FP8_CFG = dict(grid=8, embed_dim=256, num_heads=4, depth=4, tap_blocks=(1, 2), enc_dims=(64, 128, 128, 128), dec_dim=256, head_dims=(32, 1))


# ---- 1: the kernels ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host_ptr", "device_ptr"])
@pytest.mark.parametrize("ctx_dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_pack_kernels_are_exact(case, ctx_dtype, where):
    _, kind, dims, dup = case
    ctx = ctx_for("tiny", ctx_dtype)
    cdims = (C.c_int64 * len(dims))(*dims)
    n = W.dst_elems(kind, dims, dup)
    for src_dtype in SRC_DTYPES:
        src = W.source(dims, src_dtype, seed=31 + src_dtype)
        if where == "host_ptr":
            out = np.full(n, 0xAAAA if W.dst_dtype(kind) == np.uint16 else 0xAAAAAAAA, dtype=W.dst_dtype(kind))
            rc = ctx.lib.me_op_weight_pack(ctx.handle, kind, dup, cdims, len(dims), C.c_void_p(src.ctypes.data), src_dtype,
                                           C.c_void_p(out.ctypes.data))
            got = out
        else:
            s = torch.from_numpy(src.view(np.uint8).reshape(-1).copy()).cuda()
            # guard words around the destination: the kernel writes its elements and nothing else
            elem = 2 if W.dst_dtype(kind) == np.uint16 else 4
            d = torch.full((n * elem + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()                        # torch's fill runs on its own stream, the op on the context's
            rc =ctx.lib.me_op_weight_pack(ctx.handle, kind, dup, cdims, len(dims), C.c_void_p(s.data_ptr()), src_dtype,
                                           C.c_void_p(d.data_ptr() + 32))
            ctx.synchronize()
            raw = d.cpu().numpy()
            assert (raw[:32] == 0x5A).all() and (raw[32 + n * elem:] == 0x5A).all()
            got = raw[32:32 + n * elem].copy().view(W.dst_dtype(kind))
        assert rc == 0, ctx.lib.me_last_error(ctx.handle)
        W.check(got, kind, dims, dup, src, src_dtype, ctx_dtype)


def test_pack_op_errors():
    ctx = ctx_for("tiny", "f16")
    buf = np.zeros(4096, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def call(kind, dims, src=p, dst=p, sd=0):
        cd = (C.c_int64 * len(dims))(*dims)
        return ctx.lib.me_op_weight_pack(ctx.handle, kind, 0, cd, len(dims), src, sd, dst)
    assert call(W.K_MAT_16, (2, 3)) == 0
    assert call(W.K_MAT_16, (2, 3), src=None) == ME_ERR_BAD_ARG and call(W.K_MAT_16, (2, 3), dst=None) == ME_ERR_BAD_ARG
    assert call(W.K_MAT_16, (2, 3), sd=9) == ME_ERR_BAD_ARG
    assert call(W.K_CONVT_16, (2, 3, 3, 3)) == ME_ERR_BAD_SHAPE and call(W.K_CONV_16, (1, 1, 9, 9)) == ME_ERR_BAD_SHAPE
    assert call(9, (2, 3)) == ME_ERR_BAD_SHAPE
    assert ctx.lib.me_ctx_set_weight_packer(ctx.handle, 2) == ME_ERR_BAD_ARG


# ---- 2: the whole model -----------------------------------------------------------------------------------------------------

def _arena(ctx):
    ctx.synchronize()
    return ctx.weight_arena_tensor().cpu().numpy().copy()


def _depth(ctx, cfg):
    rgb = synthetic_images(1, cfg.img_size, "structured", seed=5)
    return ctx.extract_depth(rgb, None, want_fov=True)


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """the tiny synthetic checkpoint as an f16 and as an f32 torch.save file"""
    d = tmp_path_factory.mktemp("weight_pack_ckpt")
    out = {}
    for name, dt in (("f16", torch.float16), ("f32", torch.float32)):
        out[name] = str(d / f"tiny_{name}.pt")
        torch.save({k: torch.as_tensor(v).to(dt) for k, v in weights_for("tiny").items()}, out[name])
    return out


@pytest.fixture(scope="module")
def reference(checkpoints):
    """(arena bytes, depth, fov) of the host packer per (context dtype, checkpoint dtype): computed once"""
    cfg = m.ModelConfig.tiny()
    out = {}
    for dtype in ("f16", "bf16"):
        for ck in ("f16", "f32"):
            ctx = m.Context(0, dtype, cfg)
            ctx.load_checkpoint_pt(checkpoints[ck])
            rep, _ = ctx.last_weight_load()
            assert rep["where"] == "pt-host" and rep["tensors"] == len(ctx.expected_weights())
            out[(dtype, ck)] = (_arena(ctx),) + tuple(_depth(ctx, cfg))
            ctx.close()
    return out


@pytest.mark.parametrize("ck", ["f16", "f32"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_device_packed_arena_is_the_host_packers(checkpoints, reference, dtype, ck):
    cfg = m.ModelConfig.tiny()
    ctx = m.Context(0, dtype, cfg, weight_packer="device")
    ctx.load_checkpoint_pt(checkpoints[ck])
    rep, ms = ctx.last_weight_load()
    assert rep["where"] == "pt-device" and rep["tensors"] == len(ctx.expected_weights())
    assert rep["bytes_read"] == rep["bytes_uploaded"] > 0 and ms["stage"] > 0 and ms["upload"] > 0 and ms["cache_write"] == 0
    want_arena, want_depth, want_fov = reference[(dtype, ck)]
    got = _arena(ctx)
    assert got.shape == want_arena.shape
    assert np.array_equal(got, want_arena), f"first differing byte at {np.flatnonzero(got != want_arena)[:4]}"
    depth, fov = _depth(ctx, cfg)
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)) and np.array_equal(fov, want_fov)
    ctx.close()


def test_fp8_context_gives_the_same_depth_bits():
    cfg = m.ModelConfig(**FP8_CFG)
    state = synthetic_checkpoint(cfg)
    rgb = synthetic_images(1, cfg.img_size, "structured", seed=5)
    maps = []
    for packer in ("host", "device"):
        ctx = m.Context(0, "fp8", cfg, weight_packer=packer)
        ctx.load_state_dict(state)
        maps.append((_arena(ctx), ctx.extract_depth(rgb, None)))
        ctx.close()
    assert np.array_equal(maps[0][0], maps[1][0])
    assert np.array_equal(maps[0][1].view(np.uint32), maps[1][1].view(np.uint32))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_state_dict_from_cuda_tensors_and_overwritten_host_buffers(reference, dtype):
    cfg = m.ModelConfig.tiny()
    state = weights_for("tiny")
    want = reference[(dtype, "f16")][0]
    # CUDA tensors: packed where they lie
    ctx = m.Context(0, dtype, cfg, weight_packer="device")
    ctx.load_state_dict({k: torch.as_tensor(v).cuda() for k, v in state.items()})
    assert np.array_equal(_arena(ctx), want)
    # ... and as f32 CUDA tensors against f32 CPU tensors (the f16 values are exact in f32: the same arena)
    ctx.load_state_dict({k: torch.as_tensor(v).float().cuda() for k, v in state.items()})
    assert np.array_equal(_arena(ctx), want)
    ctx.close()
    # host buffers overwritten right after me_load_weight returns: the call has taken its copy
    ctx = m.Context(0, dtype, cfg, weight_packer="device")
    for name, t in state.items():
        a = np.ascontiguousarray(torch.as_tensor(t).numpy()).copy()
        dims = (C.c_int64 * a.ndim)(*a.shape)
        ctx._check(ctx.lib.me_load_weight(ctx.handle, name.encode(), C.c_void_p(a.ctypes.data), 1, dims, a.ndim))
        a.view(np.uint16)[...] = 0x7E00
    ctx._check(ctx.lib.me_weights_finalize(ctx.handle))
    assert np.array_equal(_arena(ctx), want)
    ctx.close()


def test_reloading_weights_drops_the_captured_graph():
    cfg = m.ModelConfig.tiny()
    state = weights_for("tiny")
    ctx = m.Context(0, "f16", cfg, weight_packer="device")
    ctx.load_state_dict(state)
    ctx.set_graph(True)
    rgb = torch.from_numpy(synthetic_images(1, cfg.img_size)).cuda()
    out = torch.empty(1, cfg.img_size, cfg.img_size, dtype=torch.float32, device="cuda")
    f_norm = torch.tensor([0.9], device="cuda")
    for _ in range(3):
        ctx.extract_depth(rgb, f_norm, out=out)
        ctx.synchronize()
    n0 = ctx.graph_launch_count
    assert n0 >= 2
    first = out.clone()
    other = {k: (torch.as_tensor(v) * (0.5 if k == "head.4.weight" else 1.0)).to(torch.float16) for k, v in state.items()}
    ctx.load_state_dict(other)
    ctx.extract_depth(rgb, f_norm, out=out)                  # eager again: the graph went with the old weights
    ctx.synchronize()
    assert ctx.graph_launch_count == n0 and not torch.equal(out, first)
    ctx.close()


# ---- 3: the cache -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_cache_round_trip(tmp_path, checkpoints, reference, dtype):
    cfg = m.ModelConfig.tiny()
    ctx = m.Context(0, dtype, cfg, weight_packer="device")
    ctx.load_checkpoint_pt(checkpoints["f16"])
    path = str(tmp_path / "arena.mearena")
    ctx.save_weight_arena(path, checkpoints["f16"])
    assert os.path.getsize(path) == 256 + ctx.weight_arena_bytes() and glob.glob(str(tmp_path / "*.tmp.*")) == []
    assert ctx.last_weight_load()[1]["cache_write"] > 0
    ctx.close()
    fresh = m.Context(0, dtype, cfg)
    fresh.load_weight_arena(path, checkpoints["f16"])
    rep, ms = fresh.last_weight_load()
    assert rep["where"] == "cache" and rep["bytes_read"] == os.path.getsize(path) and rep["bytes_uploaded"] == fresh.weight_arena_bytes()
    want_arena, want_depth, want_fov = reference[(dtype, "f16")]
    assert np.array_equal(_arena(fresh), want_arena)
    depth, fov = _depth(fresh, cfg)
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)) and np.array_equal(fov, want_fov)
    fresh.close()


def test_damaged_cache_is_refused_and_leaves_the_context_unloaded(tmp_path, checkpoints):
    cfg = m.ModelConfig.tiny()
    ctx = m.Context(0, "f16", cfg)
    ctx.load_checkpoint_pt(checkpoints["f16"])
    good = str(tmp_path / "good.mearena")
    ctx.save_weight_arena(good)
    data = open(good, "rb").read()
    rgb = synthetic_images(1, cfg.img_size)
    out = np.empty((1, cfg.img_size, cfg.img_size), np.float32)

    def damaged(name, blob, word):
        p = str(tmp_path / name)
        open(p, "wb").write(blob)
        c = m.Context(0, "f16", cfg)
        c.load_checkpoint_pt(checkpoints["f16"])           # finalized weights: the refusal must take them away
        assert c.lib.me_load_weight_arena(c.handle, p.encode(), None) == ME_ERR_IO
        msg = c.lib.me_last_error(c.handle).decode()
        assert name in msg and "delete" in msg and word in msg, msg
        rc = c.lib.me_extract_depth_u8(c.handle, C.c_void_p(rgb.ctypes.data), 1, None, C.c_void_p(out.ctypes.data), None)
        assert rc == ME_ERR_NOT_READY
        assert c.lib.me_weights_finalize(c.handle) == 3    # ME_ERR_MISSING_WEIGHT: every slot is marked not loaded
        c.load_checkpoint_pt(checkpoints["f16"])           # ... and the context is still usable
        c.close()

    flipped = bytearray(data)
    flipped[256 + len(data) // 2] ^= 0x10
    damaged("flipped.mearena", bytes(flipped), "checksum")
    damaged("truncated.mearena", data[:-4096], "short")
    damaged("header_only.mearena", data[:100], "short")
    magic = bytearray(data)
    magic[3] ^= 0xFF
    damaged("magic.mearena", bytes(magic), "magic")
    damaged("longer.mearena", data + b"\0" * 8, "longer")
    # a cache of a context with another split_operands: another name, and refused when renamed into place
    other = m.Context(0, "f16", dataclasses.replace(m.ModelConfig.tiny(), split_operands=0))
    assert other.weight_cache_path(checkpoints["f16"]) != ctx.weight_cache_path(checkpoints["f16"])
    other.load_checkpoint_pt(checkpoints["f16"])
    theirs = str(tmp_path / "theirs.mearena")
    other.save_weight_arena(theirs)
    other.close()
    damaged("theirs.mearena", open(theirs, "rb").read(), "not this context's")
    ck2 = str(tmp_path / "tiny.pt")
    shutil.copy(checkpoints["f16"], ck2)
    shutil.copy(theirs, ctx.weight_cache_path(ck2))        # renamed into this context's place: the policy refuses it too
    assert ctx.lib.me_load_checkpoint_cached(ctx.handle, ck2.encode(), 0, None) == ME_ERR_IO
    assert "delete" in ctx.lib.me_last_error(ctx.handle).decode()
    ctx.close()


def test_cached_checkpoint_policy(tmp_path, capfd):
    cfg = m.ModelConfig.tiny()
    ckpt = str(tmp_path / "tiny.pt")
    tiny_checkpoint(ckpt)
    ctx = m.Context(0, "f16", cfg, weight_packer="device")
    cache = ctx.weight_cache_path(ckpt)
    assert os.path.dirname(cache) == str(tmp_path) and os.path.basename(cache).startswith("tiny-f16-") and cache.endswith(".mearena")
    assert os.path.basename(cache) == "tiny-f16-%016x.mearena" % ctx.weight_arena_layout()
    # no cache, no flag: the .pt, and nothing is written
    assert ctx.load_checkpoint_cached(ckpt, False) == "pt-device" and not os.path.exists(cache)
    want = _arena(ctx)
    # with the flag the cache is written, and the next load takes it
    assert ctx.load_checkpoint_cached(ckpt, True) == "pt-device" and os.path.exists(cache)
    assert ctx.load_checkpoint_cached(ckpt, False) == "cache" and ctx.last_weight_load()[0]["where"] == "cache"
    assert np.array_equal(_arena(ctx), want)
    capfd.readouterr()
    # a touched .pt makes it stale: one line, the .pt is loaded, the cache stays as it is without the flag
    before = os.stat(cache).st_mtime_ns
    st = os.stat(ckpt)
    os.utime(ckpt, ns=(st.st_atime_ns, st.st_mtime_ns + 5_000_000_000))
    assert ctx.load_checkpoint_cached(ckpt, False) == "pt-device"
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "stale" in err and os.path.basename(cache) in err
    assert os.stat(cache).st_mtime_ns == before
    # with the flag it is rewritten, and a second load uses it
    assert ctx.load_checkpoint_cached(ckpt, True) == "pt-device"
    assert "stale" in capfd.readouterr().err
    assert ctx.load_checkpoint_cached(ckpt, False) == "cache" and capfd.readouterr().err == ""
    # the .pt may be gone
    os.remove(ckpt)
    assert ctx.load_checkpoint_cached(ckpt, False) == "cache"
    assert np.array_equal(_arena(ctx), want)
    # a damaged cache is an error that names the file, not a silent reload
    blob = bytearray(open(cache, "rb").read())
    blob[-1] ^= 1
    open(cache, "wb").write(bytes(blob))
    where = C.c_int32()
    assert ctx.lib.me_load_checkpoint_cached(ctx.handle, ckpt.encode(), 0, C.byref(where)) == ME_ERR_IO
    assert os.path.basename(cache) in ctx.lib.me_last_error(ctx.handle).decode()
    ctx.close()


# ---- 4: both command lines --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["compiled", "python"])
def test_convert_checkpoints_in_the_command_lines(tmp_path, which):
    from PIL import Image
    assert os.path.exists(CLI), "the compiled command line is built by __graft_entry__.build()"
    S = m.ModelConfig.tiny().img_size
    work, fresh = tmp_path / "work", tmp_path / "fresh"
    work.mkdir(), fresh.mkdir()
    src = str(tmp_path / "photo.png")
    Image.fromarray(synthetic_images(1, S, "structured", seed=11)[0]).save(src)
    argv = [CLI] if which == "compiled" else [sys.executable, "-m", "matrix_eyes_amd"]
    base = dict(os.environ, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_SEED="7", PYTHONPATH=ROOT)
    base.pop("MATRIX_EYES_WEIGHT_PACKER", None)

    def run(folder, out, *flags, env=base, expect=0):
        return run_cli(argv + [f"--checkpoint-path={folder / 'tiny.pt'}", "--focal-length=35", *flags, src, str(tmp_path / out)], env, expect)

    tiny_checkpoint(str(work / "tiny.pt"))
    tiny_checkpoint(str(fresh / "tiny.pt"))
    run(work, "first.png", "--convert-checkpoints", env=dict(base, MATRIX_EYES_WEIGHT_PACKER="device"))
    caches = glob.glob(str(work / "*.mearena"))
    assert len(caches) == 1 and sorted(os.listdir(work)) == sorted(["tiny.pt", os.path.basename(caches[0])])
    first = open(tmp_path / "first.png", "rb").read()
    run(work, "second.png")
    assert open(tmp_path / "second.png", "rb").read() == first
    os.remove(work / "tiny.pt")
    run(work, "third.png")
    assert open(tmp_path / "third.png", "rb").read() == first
    run(fresh, "plain.png")                                 # no flag, no cache: nothing is created
    assert os.listdir(fresh) == ["tiny.pt"] and open(tmp_path / "plain.png", "rb").read() == first
    r = run(fresh, "x.png", env=dict(base, MATRIX_EYES_WEIGHT_PACKER="fpga"), expect=1 if which == "compiled" else 2)
    assert "MATRIX_EYES_WEIGHT_PACKER" in r.stdout + r.stderr and not (tmp_path / "x.png").exists()
