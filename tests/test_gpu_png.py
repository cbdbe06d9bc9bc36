"""GPU tests of the PNG encoder (me_png_encode_rgb8, me_output_png, me_output_depth_map_png, me_output_stereogram_png):
the device's files are read back by tests/png_check.py and by Pillow to exactly the input pixels, every row's filter
byte is the rule's, the stream structure survives chunk boundaries, the file is never worse than stored, it
compresses, it is deterministic, it chains on the device, and both command lines write it on request.

One context for the module; the 12-megapixel pictures are encoded once each."""
import ctypes as C
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_check as P       # noqa: E402
import png_pictures as pic  # noqa: E402

import matrix_eyes_amd as m  # noqa: E402
from util import run_cli, tiny_checkpoint  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
BIG = (3024, 4032)   # rows, columns of the 4032 x 3024 picture
ME_RESIZE_MAX_DIM = 16384


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0, "f16", m.ModelConfig.tiny())   # no weights: the encoder needs a context only
    yield c
    c.close()


@pytest.fixture(scope="module")
def field():
    return pic.inverse_depth_field(1536)


def _decode_both(data: bytes, rgb: np.ndarray):
    """png_check and Pillow read `data` back to rgb; returns the filter bytes"""
    from PIL import Image
    px, types = P.read_png(data)
    assert px.shape == rgb.shape and np.array_equal(px, rgb)
    pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(pil, rgb)
    return types


def _check(ctx, rgb, device_pointer=False):
    """encode (host or device pointer), decode with both readers, compare the filter bytes with the rule; -> the file"""
    if device_pointer:
        data = ctx.png_encode(torch.from_numpy(rgb).cuda()).cpu().numpy().tobytes()
    else:
        data = ctx.png_encode(rgb)
    types = _decode_both(data, rgb)
    assert np.array_equal(types, P.choose_filters(rgb))
    return data


def _host_file_size(rgb):
    """The host layer's encode_png: filter byte 0 in front of every row, compress2 level 6 (+ the container)."""
    h = rgb.shape[0]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, -1)], axis=1)
    return len(zlib.compress(rows.tobytes(), 6)) + 57


# ---- 1, 2: pixels exact and filter bytes, small shapes and both pointer kinds ---------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (7, 1), (1, 7), (61, 97), (129, 257)])
def test_small_shapes(ctx, shape):
    h, w = shape
    for k, rgb in enumerate((pic.noise_picture(h, w, seed=h + w), pic.stereogram_like(h, w, pattern=max(2, w // 5)),
                             pic.flat_picture(h, w), pic.checkerboard(h, w))):
        a = _check(ctx, rgb, device_pointer=False)
        b = _check(ctx, rgb, device_pointer=True)
        assert a == b, k


def test_shapes_around_a_whole_number_of_chunks(ctx):
    shapes = pic.around_chunks()
    assert sorted(shapes) == [-1, 0, 1]
    for delta, (h, w) in shapes.items():
        assert (h * (3 * w + 1) - delta) % 65536 == 0
        _check(ctx, pic.noise_picture(h, w, seed=delta + 5))
        _check(ctx, pic.stereogram_like(h, w, pattern=120), device_pointer=True)


# ---- the depth pictures (1, 2, 5) ---------------------------------------------------------------------------------------

def test_depth_picture_native(ctx, field):
    dm = m.DepthMap(ctx, field, (1536, 1536))
    rgb = dm.depth_map_rgb_resized()
    assert rgb.shape == (1536, 1536, 3)
    data = _check(ctx, rgb, device_pointer=True)
    host = _host_file_size(rgb)
    print(f"depth 1536x1536: device file {len(data)} bytes, host file {host} bytes, ratio {len(data) / host:.3f}")
    assert len(data) <= 2 * host


def test_depth_picture_resized(ctx, field):
    dm = m.DepthMap(ctx, field, (4032, 3024))
    rgb = dm.depth_map_rgb_resized()
    assert rgb.shape == BIG + (3,)
    data = _check(ctx, rgb)
    host = _host_file_size(rgb)
    print(f"depth 4032x3024: device file {len(data)} bytes, host file {host} bytes, ratio {len(data) / host:.3f}")
    assert len(data) <= 2 * host


def test_stereogram_picture(ctx, field):
    dm = m.DepthMap(ctx, field, (4032, 3024))
    noise = pic.noise_picture(BIG[0], BIG[1], seed=21)
    rgb = dm.stereogram(None, 1.0 / 16.0, noise)
    assert rgb.shape == BIG + (3,)
    data = _check(ctx, rgb, device_pointer=True)
    print(f"stereogram 4032x3024: device file {len(data)} bytes, {len(data) / rgb.size:.3f} x raw")
    assert len(data) <= 0.5 * rgb.size


# ---- 4: never worse than stored -------------------------------------------------------------------------------------------

def test_noise_is_never_worse_than_stored(ctx):
    for h, w, dev in ((BIG[0], BIG[1], False), (61, 97, True)):
        rgb = pic.noise_picture(h, w, seed=33)
        data = _check(ctx, rgb, device_pointer=dev)
        cap = 1.001 * h * (3 * w + 1) + 1024
        print(f"noise {w}x{h}: file {len(data)} bytes, {len(data) / (h * (3 * w + 1)):.5f} x the filtered stream")
        assert len(data) <= cap


# ---- 3: structure -----------------------------------------------------------------------------------------------------------

def test_transposed_shape_and_long_matches(ctx):
    """3024 x 4032, flat in its upper half (matches of length 258 end to end, reaching back across chunk boundaries)
    and a one-pixel checkerboard below: chunk boundaries fall inside matches and inside rows (3 * 3024 + 1 bytes a row)."""
    h, w = BIG[1], BIG[0]
    rgb = pic.checkerboard(h, w)
    rgb[: h // 2] = 0
    data = _check(ctx, rgb, device_pointer=True)
    assert len(data) < 0.01 * rgb.size


def test_flat_pictures(ctx):
    for rgb in (pic.flat_picture(600, 1000), pic.checkerboard(601, 999)):
        data = _check(ctx, rgb)
        assert len(data) < 0.02 * rgb.size


def test_nothing_reaches_past_the_window(ctx):
    rgb = pic.alternating_rows()
    data = _check(ctx, rgb)                          # a distance of 80 KB written as a match would not inflate
    assert len(data) <= 1.001 * rgb.shape[0] * (3 * rgb.shape[1] + 1) + 1024


# ---- 6: deterministic -------------------------------------------------------------------------------------------------------

def test_deterministic_and_scratch_reuse(ctx):
    a_rgb, b_rgb = pic.depth_picture(700), pic.stereogram_like(333, 801, pattern=90)
    a1 = ctx.png_encode(a_rgb)
    a2 = ctx.png_encode(a_rgb)
    b1 = ctx.png_encode(b_rgb)                       # a different size in between: the scratch is reused
    a3 = ctx.png_encode(a_rgb)
    b2 = ctx.png_encode(torch.from_numpy(b_rgb).cuda()).cpu().numpy().tobytes()
    assert a1 == a2 == a3 and b1 == b2
    _decode_both(a1, a_rgb)
    _decode_both(b1, b_rgb)


# ---- 7: chained on the device -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [0, 1])
def test_chained_on_the_device(ctx, field, overlap):
    size = (1000, 750)
    want = m.DepthMap(ctx, field[:512, :512].copy(), size).depth_map_rgb_resized()      # the host-pointer path
    ctx.set_output_overlap(bool(overlap))
    try:
        depth = torch.from_numpy(field[:512, :512].copy()).cuda()
        torch.cuda.synchronize()
        dd = m.DeviceDepthMap(ctx, depth, size)      # me_depth_clamp_minmax_async
        rgb = dd.depth_map_rgb_resized()             # me_depthmap_rgb_resized, device destination, not synchronised
        file = ctx.png_encode(rgb)                   # me_png_encode_rgb8 on the same stream
        data = file.cpu().numpy().tobytes()
    finally:
        ctx.set_output_overlap(False)
    _decode_both(data, want)


# ---- the file-writing calls ---------------------------------------------------------------------------------------------------

def test_output_calls_write_the_same_files(ctx, field, tmp_path):
    small = field[::3, ::3].copy()
    dm = m.DepthMap(ctx, small, (640, 480))
    rgb = dm.depth_map_rgb_resized()
    ctx.output_png(rgb, str(tmp_path / "a.png"))
    dm.output_depth_map_png(str(tmp_path / "b.png"))
    a, b = (tmp_path / "a.png").read_bytes(), (tmp_path / "b.png").read_bytes()
    assert a == b == ctx.png_encode(rgb)
    _decode_both(a, rgb)
    noise = pic.noise_picture(240, 320, seed=8)
    st = dm.stereogram(0.5, 1.0 / 16.0, noise)
    dm.output_stereogram_png(str(tmp_path / "c.png"), 0.5, 1.0 / 16.0, noise)
    _decode_both((tmp_path / "c.png").read_bytes(), st)
    # DepthMap.output_image with the encoder named
    fmt = m.ImageOutputFormat.DepthMap()
    dm.output_image(str(tmp_path / "d.png"), "", fmt, m.VertexMode.Color, resampler="device", png_encoder="device")
    assert (tmp_path / "d.png").read_bytes() == a
    dm.output_image(str(tmp_path / "e.png"), "", fmt, m.VertexMode.Color, resampler="device", png_encoder="pillow")
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "e.png")), rgb)


# ---- 8: both command lines ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["compiled", "python"])
def test_command_lines(tmp_path, which):
    from PIL import Image
    from matrix_eyes_amd.synthetic import synthetic_images
    assert os.path.exists(CLI), "the compiled command line is built by __graft_entry__.build()"
    S = m.ModelConfig.tiny().img_size
    ckpt, src = str(tmp_path / "tiny.pt"), str(tmp_path / "photo.png")
    tiny_checkpoint(ckpt)
    Image.fromarray(synthetic_images(1, S, "structured", seed=11)[0]).resize((S + 88, S - 40)).save(src)
    argv = [CLI] if which == "compiled" else [sys.executable, "-m", "matrix_eyes_amd"]
    base = dict(os.environ, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_SEED="7", PYTHONPATH=ROOT)
    base.pop("MATRIX_EYES_PNG_ENCODER", None)

    def run(env, *args, expect=0):
        return run_cli(argv + [f"--checkpoint-path={ckpt}", "--focal-length=35", *args], env, expect)

    dev = dict(base, MATRIX_EYES_PNG_ENCODER="device")
    for name, flags in (("depth", []), ("stereo", ["--image-output-format=stereogram"])):
        plain, device = str(tmp_path / f"{name}_plain.png"), str(tmp_path / f"{name}_device.png")
        run(base, *flags, src, plain)
        run(dev, *flags, src, device)
        want = np.asarray(Image.open(plain).convert("RGB"))
        assert want.shape == (S - 40, S + 88, 3)
        data = open(device, "rb").read()
        _decode_both(data, want)
        assert data != open(plain, "rb").read()                               # it is this encoder's file
        assert len(P.chunks(data)) >= 3 and data[37:41] == b"IDAT"
    r = run(dict(base, MATRIX_EYES_PNG_ENCODER="fpga"), src, str(tmp_path / "x.png"),
            expect=1 if which == "compiled" else 2)
    assert "MATRIX_EYES_PNG_ENCODER" in r.stdout + r.stderr and not (tmp_path / "x.png").exists()


# ---- 9: errors ----------------------------------------------------------------------------------------------------------------

def test_errors(ctx, tmp_path):
    lib, h = ctx.lib, ctx.handle
    rgb = pic.noise_picture(8, 8)
    p = C.c_void_p(rgb.ctypes.data)
    ptr, n = C.c_void_p(), C.c_int64()
    assert lib.me_png_encode_rgb8(h, None, 8, 8, C.byref(ptr), C.byref(n)) == 1
    assert lib.me_png_encode_rgb8(h, p, 8, 8, None, C.byref(n)) == 1
    assert lib.me_png_encode_rgb8(h, p, 8, 8, C.byref(ptr), None) == 1
    assert lib.me_output_png(h, None, 8, 8, b"x.png") == 1 and lib.me_output_png(h, p, 8, 8, None) == 1
    for w_, h_ in ((0, 8), (8, 0), (-1, 8), (8, -3), (ME_RESIZE_MAX_DIM + 1, 1), (1, ME_RESIZE_MAX_DIM + 1)):
        assert lib.me_png_encode_rgb8(h, p, w_, h_, C.byref(ptr), C.byref(n)) == 2, (w_, h_)
        assert lib.me_output_png(h, p, w_, h_, str(tmp_path / "x.png").encode()) == 2
    assert b"ME_RESIZE_MAX_DIM" in lib.me_last_error(h)
    nowhere = str(tmp_path / "no" / "such" / "dir" / "x.png").encode()
    assert lib.me_output_png(h, p, 8, 8, nowhere) == 7
    d = np.full((8, 8), 0.5, np.float32)
    dp = C.c_void_p(d.ctypes.data)
    assert lib.me_output_depth_map_png(h, None, 8, 8, 0.1, 1.0, None, 8, 8, b"x.png") == 1
    assert lib.me_output_depth_map_png(h, dp, 8, 8, 0.1, 1.0, None, 8, 8, None) == 1
    assert lib.me_output_depth_map_png(h, dp, 8, 8, 0.1, 1.0, None, 0, 8, b"x.png") == 2
    assert lib.me_output_depth_map_png(h, dp, 8, 8, 0.1, 1.0, None, 8, ME_RESIZE_MAX_DIM + 1, b"x.png") == 2
    assert lib.me_output_depth_map_png(h, dp, 8, 8, 0.1, 1.0, None, 8, 8, nowhere) == 7
    assert lib.me_output_stereogram_png(h, dp, 8, 8, 0.1, 1.0, 8, 8, 0.0625, None, b"x.png") == 1
    assert lib.me_output_stereogram_png(h, dp, 8, 8, 0.1, 1.0, 8, -8, 0.0625, p, b"x.png") == 2
    assert lib.me_output_stereogram_png(h, dp, 8, 8, 0.1, 1.0, 8, 8, 0.0625, p, nowhere) == 7
    # wrong in two ways: the first check of the entry decides; and no entry touches a missing context
    assert lib.me_output_depth_map_png(h, None, 8, 8, 0.1, 1.0, None, 0, 8, b"x.png") == 1
    assert lib.me_output_png(None, p, 8, 8, b"x.png") == 1
    assert lib.me_output_depth_map_png(None, dp, 8, 8, 0.1, 1.0, None, 8, 8, b"x.png") == 1
    assert lib.me_output_stereogram_png(None, dp, 8, 8, 0.1, 1.0, 8, 8, 0.0625, p, b"x.png") == 1
    with pytest.raises(m.MatrixEyesError):
        ctx.png_encode(np.zeros((4, 4), np.uint8))
    # the context still works
    _check(ctx, rgb)
    ctx.output_png(rgb, str(tmp_path / "ok.png"))
    _decode_both((tmp_path / "ok.png").read_bytes(), rgb)
