"""GPU tests of the Lanczos3 resampler (csrc/resample.hip behind me_resize_lanczos3_rgb8 / me_depthmap_rgb_resized):
byte-identical to oracle/image_oracle.c -- the `image` crate's sampler that reconstruction.rs:107-113, output.rs:133-137
and output.rs:206-218 call -- for every size pair, through host and device pointers, chained with the model and the
colour map, and through both command lines.  Every comparison is np.array_equal: there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from oracle import output_oracle as OO
from util import ctx_for, loaded_ctx, ptr, run_cli, tiny_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
_ORACLE = None

CASES = [((4032, 3024), (1536, 1536)), ((3024, 4032), (1536, 1536)), ((1536, 1536), (4032, 3024)),
         ((6000, 4000), (1536, 1536)), ((1536, 1536), (1537, 1535)), ((1536, 1536), (97, 61)),
         ((301, 199), (97, 333)), ((64, 48), (1536, 1536)), ((40, 30), (1, 1)), ((1536, 8), (1, 8)),
         ((1, 7), (5, 3)), ((257, 129), (256, 128)), ((100, 100), (100, 100))]


def oracle_resize(img, nw, nh):
    global _ORACLE
    if _ORACLE is None:
        OO.build()
        _ORACLE = C.CDLL(os.path.join(ROOT, "oracle", "_build", "libimage_oracle.so"))
    h, w, _ = img.shape
    a = np.ascontiguousarray(img)
    want = np.empty((nh, nw, 3), np.uint8)
    assert _ORACLE.oracle_resize_lanczos3_rgb8(C.c_void_p(a.ctypes.data), C.c_int64(w), C.c_int64(h),
                                               C.c_void_p(want.ctypes.data), C.c_int64(nw), C.c_int64(nh)) == 0
    return want


def photo(w, h, seed):
    """tests/test_host_cpp.py's kind of picture (smooth, noisy, colourful) with hard 0 / 255 edges: overshoot clamps"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([127 + 100 * np.sin(x / 17.0 + y / 29.0), 127 + 100 * np.cos(x / 11.0 - y / 23.0),
                  127 + 90 * np.sin((x + y) / 31.0)], -1) + rng.normal(0, 6, (h, w, 3)).astype(np.float32)
    img = np.clip(a, 0, 255).astype(np.uint8)
    for _ in range(12):                                       # blocks and lines of pure black / white
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y0:y0 + int(rng.integers(1, max(2, h // 6))), x0:x0 + int(rng.integers(1, max(2, w // 6)))] = 255 * int(rng.integers(0, 2))
    return img


def picture(index, w, h):
    """photos with hard edges for half of the cases, uniform random bytes for the rest"""
    if index % 2 == 1:
        return photo(w, h, 100 + index)
    return np.random.default_rng(200 + index).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    return ctx_for("tiny", "f16")         # a context is enough: no weights are loaded for a resize


@pytest.mark.parametrize("index", range(len(CASES)), ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in CASES])
def test_resize_equals_the_oracle(ctx, index):
    (w, h), (nw, nh) = CASES[index]
    img = picture(index, w, h)
    want = oracle_resize(img, nw, nh)
    got = ctx.resize_lanczos3(img, (nw, nh))                  # host pointers
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = int((got != want).sum())
    print(f"{w}x{h} -> {nw}x{nh}: {bad} of {want.size} bytes differ; saturated low/high "
          f"{float((want == 0).mean()):.4f}/{float((want == 255).mean()):.4f}")
    assert np.array_equal(got, want)
    dev = ctx.resize_lanczos3(torch.from_numpy(img).cuda(), (nw, nh))   # device pointers, nothing crosses to the host
    assert dev.is_cuda and dev.dtype == torch.uint8
    ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want)


def test_two_size_pairs_back_to_back(ctx):
    """two different pairs queued on the stream without a synchronise between them: the second call's tables and
    intermediate must not reach the first call's kernels"""
    a, b = picture(0, 640, 480), picture(1, 333, 517)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    oa = torch.empty((200, 300, 3), dtype=torch.uint8, device="cuda")
    ob = torch.empty((1024, 777, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.handle
    assert lib.me_resize_lanczos3_rgb8(hd, ptr(da), 640, 480, ptr(oa), 300, 200) == 0
    assert lib.me_resize_lanczos3_rgb8(hd, ptr(db), 333, 517, ptr(ob), 777, 1024) == 0
    assert lib.me_ctx_synchronize(hd) == 0
    assert np.array_equal(oa.cpu().numpy(), oracle_resize(a, 300, 200))
    assert np.array_equal(ob.cpu().numpy(), oracle_resize(b, 777, 1024))


def test_unaligned_device_pointers(ctx):
    """a source and a destination that start at odd addresses: the byte-wide vertical path and the head / tail of the
    packed stores"""
    img = picture(1, 120, 37)
    src = torch.zeros(img.size + 8, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 * 51 * 3 + 8,), 77, dtype=torch.uint8, device="cuda")
    src[1:1 + img.size] = torch.from_numpy(img).cuda().flatten()
    s, d = src[1:], dst[3:]
    assert ctx.lib.me_resize_lanczos3_rgb8(ctx.handle, C.c_void_p(s.data_ptr()), 120, 37, C.c_void_p(d.data_ptr()), 64, 51) == 0
    ctx.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out[3:3 + 64 * 51 * 3].reshape(51, 64, 3), oracle_resize(img, 64, 51))
    assert (out[:3] == 77).all() and (out[3 + 64 * 51 * 3:] == 77).all()          # nothing written around it


def test_table_cache_turns_over(ctx):
    """more size pairs than the context keeps tables for, then the first ones again"""
    img = picture(0, 96, 64)
    sizes = [(40 + 3 * k, 30 + 5 * k) for k in range(24)]
    for rounds in range(2):
        for nw, nh in sizes:
            assert np.array_equal(ctx.resize_lanczos3(img, (nw, nh)), oracle_resize(img, nw, nh)), (rounds, nw, nh)


def test_chain_resize_then_model():
    """reconstruction.rs:107-124 chained on the stream: the resize into a device buffer, me_extract_depth_u8 on that
    pointer -- against the oracle's resize on the host handed to the same entry"""
    ctx = loaded_ctx("tiny", "f16")
    S = ctx.cfg.img_size
    img = photo(300, 200, 5)
    resized = torch.empty((1, S, S, 3), dtype=torch.uint8, device="cuda")
    depth = torch.empty((1, S, S), dtype=torch.float32, device="cuda")
    fov = torch.empty((1,), dtype=torch.float32, device="cuda")
    lib, hd = ctx.lib, ctx.handle
    assert lib.me_resize_lanczos3_rgb8(hd, C.c_void_p(img.ctypes.data), 300, 200, ptr(resized), S, S) == 0
    assert lib.me_extract_depth_u8(hd, ptr(resized), 1, None, ptr(depth), ptr(fov)) == 0
    ctx.synchronize()
    want_depth, want_fov = ctx.extract_depth(oracle_resize(img, S, S)[None], None, want_fov=True)
    assert np.array_equal(depth.cpu().numpy(), want_depth)
    assert np.array_equal(fov.cpu().numpy(), want_fov)


@pytest.mark.parametrize("case", [(1536, (4032, 3024)), (96, (300, 200))])
def test_depthmap_rgb_resized(ctx, case):
    """output.rs:123-137: me_depthmap_rgb_resized == me_depthmap_rgb, then the oracle's resize; with the range as two
    scalars and as me_depth_clamp_minmax_async left it on the device"""
    side, (ow, oh) = case
    rng = np.random.default_rng(side)
    depth = rng.uniform(0.002, 12.0, (side, side)).astype(np.float32)       # clamped to [1/250, 10] by DepthMap::new
    dm = m.DepthMap(ctx, depth, (ow, oh))
    mn, mx = dm.inverse_depth_range()
    want = oracle_resize(dm.depth_map_rgb(), ow, oh)
    assert np.array_equal(dm.depth_map_rgb_resized(), want)
    d = torch.from_numpy(depth).cuda()
    mm = torch.empty(2, dtype=torch.float32, device="cuda")
    out = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
    lib, hd = ctx.lib, ctx.handle
    assert lib.me_depth_clamp_minmax_async(hd, ptr(d), d.numel(), ptr(mm)) == 0
    assert lib.me_depthmap_rgb_resized(hd, ptr(d), side, side, 0.0, 0.0, ptr(mm), ow, oh, ptr(out)) == 0
    ctx.synchronize()
    assert mm.tolist() == [mn, mx]
    assert np.array_equal(out.cpu().numpy(), want)
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(depth).cuda(), (ow, oh))            # the same through the Python mirror
    got = ddm.depth_map_rgb_resized()
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_argument_errors_leave_the_context_usable(ctx):
    lib, hd = ctx.lib, ctx.handle
    img = picture(1, 40, 30)
    want = oracle_resize(img, 20, 10)
    out = np.empty((10, 20, 3), np.uint8)
    src, dst = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    big = np.zeros(40 * 30 * 3 + 64, np.uint8)
    depth = np.full((8, 8), 0.5, np.float32)
    dp = C.c_void_p(depth.ctypes.data)

    def good():
        out[:] = 0
        assert lib.me_resize_lanczos3_rgb8(hd, src, 40, 30, dst, 20, 10) == 0
        assert np.array_equal(out, want)

    bad_arg, bad_shape = 1, 2
    calls = [
        (lambda: lib.me_resize_lanczos3_rgb8(hd, None, 40, 30, dst, 20, 10), bad_arg),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 40, 30, None, 20, 10), bad_arg),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 40, 30, src, 20, 10), bad_arg),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, C.c_void_p(big.ctypes.data), 40, 30, C.c_void_p(big.ctypes.data + 100), 20, 10), bad_arg),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 0, 30, dst, 20, 10), bad_shape),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 40, -1, dst, 20, 10), bad_shape),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 40, 30, dst, 0, 10), bad_shape),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 40, 30, dst, 20, 1 << 20), bad_shape),
        (lambda: lib.me_resize_lanczos3_rgb8(hd, src, 1 << 20, 30, dst, 20, 10), bad_shape),
        (lambda: lib.me_depthmap_rgb_resized(hd, None, 8, 8, 0.1, 1.0, None, 20, 10, dst), bad_arg),
        (lambda: lib.me_depthmap_rgb_resized(hd, dp, 8, 8, 0.1, 1.0, None, 20, 10, None), bad_arg),
        (lambda: lib.me_depthmap_rgb_resized(hd, dp, 8, 8, 0.1, 1.0, dp, 20, 10, dst), bad_arg),   # a host range
        (lambda: lib.me_depthmap_rgb_resized(hd, dp, 8, 0, 0.1, 1.0, None, 20, 10, dst), bad_shape),
        (lambda: lib.me_depthmap_rgb_resized(hd, dp, 8, 8, 0.1, 1.0, None, 20, 1 << 20, dst), bad_shape),
    ]
    good()
    for k, (call, code) in enumerate(calls):
        assert call() == code, k
        assert lib.me_last_error(hd)
        good()
    assert lib.me_resize_lanczos3_rgb8(None, src, 40, 30, dst, 20, 10) == bad_arg        # no crash without a context
    assert lib.me_depthmap_rgb_resized(None, dp, 8, 8, 0.1, 1.0, None, 20, 10, dst) == bad_arg
    with pytest.raises(m.MatrixEyesError):
        m.depth_pro.resolve_resampler("bicubic")


def test_command_lines_agree(tmp_path):
    """Compiled CLI, tiny model, a 300 x 200 PNG photo: the depth PNG and the vertex-coloured PLY are the same files
    with MATRIX_EYES_RESAMPLER=host (the loop on one CPU core) and without it (the GPU); and the Python mirror with
    resampler="device" writes the same depth pixels, which it does not with Pillow's filter."""
    from PIL import Image
    from matrix_eyes_amd import reconstruction as R
    cfg = m.ModelConfig.tiny()
    ckpt = str(tmp_path / "tiny.pt")
    tiny_checkpoint(ckpt)
    src = str(tmp_path / "photo.png")
    Image.fromarray(photo(300, 200, 9)).save(src)
    base = {k: v for k, v in os.environ.items() if k != "MATRIX_EYES_RESAMPLER"}

    def cli(out, *args, **extra):
        run_cli([CLI, f"--checkpoint-path={ckpt}", "--focal-length=35", *args, src, str(tmp_path / out)],
                dict(base, MATRIX_EYES_MODEL="tiny", **extra), timeout=300)
        return (tmp_path / out).read_bytes()

    depth_dev = cli("depth_dev.png")
    depth_host = cli("depth_host.png", MATRIX_EYES_RESAMPLER="host")
    assert depth_dev == depth_host and len(depth_dev) > 1000
    ply_dev = cli("mesh_dev.ply", "--mesh=vertex-colors")
    ply_host = cli("mesh_host.ply", "--mesh=vertex-colors", MATRIX_EYES_RESAMPLER="host")
    assert ply_dev == ply_host and len(ply_dev) > 1000
    r = run_cli([CLI, f"--checkpoint-path={ckpt}", src, str(tmp_path / "x.png")],
                dict(base, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_RESAMPLER="gpu"), expect=None, timeout=300)
    assert r.returncode != 0 and "MATRIX_EYES_RESAMPLER" in r.stdout + r.stderr          # not a silent default

    loader = m.DepthProModelLoader(ckpt, False, cfg)
    R.extract_depth(0, loader, src, str(tmp_path / "depth_py.png"), 35.0, m.ImageOutputFormat.DepthMap(),
                    m.VertexMode.Color, resampler="device")
    cpp, py = np.asarray(Image.open(tmp_path / "depth_dev.png")), np.asarray(Image.open(tmp_path / "depth_py.png"))
    assert cpp.shape == py.shape == (200, 300, 3)
    assert np.array_equal(cpp, py)
