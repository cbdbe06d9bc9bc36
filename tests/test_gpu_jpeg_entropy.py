"""GPU tests of the device entropy decoder (csrc/jpeg_entropy.hip): me_op_jpeg_entropy gives exactly the coefficients of the
host decoder (me_op_jpeg_coefficients_host) without declining, at the default subsequence length, at 128 bits and at the
smallest one, where one small picture spans several workgroups; with me_ctx_set_jpeg_entropy(ctx, 1) the pictures of
me_jpeg_decode_rgb8 / me_jpeg_decode_resized_rgb8 stay the host decoder's bytes; files the device decoder declines take the
host decoder, whose pixels or words stand; both command lines write the same files with MATRIX_EYES_JPEG_ENTROPY=device and
=host.  Every comparison is np.array_equal: there is no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from util import ctx_for, ptr, run_cli, tiny_checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_files as J  # noqa: E402
import jpeg_entropy_files as E  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = J.ROOT
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
SMALLEST = 64
DECLINED = 100                         # ME_OP_JPEG_ENTROPY_DECLINED
BAD_ARG = 1
SEQUENTIAL = E.sequential_files()
AT_128 = ("123x77-s2-base-q95", "517x333-s2", "grey", "restart-rows", "restart-blocks", "s440", "s411")
_HOST = {}


@pytest.fixture(scope="module")
def ctx():
    return ctx_for("tiny", "f16")         # a context is enough: no weights are loaded for a decode


@pytest.fixture
def device_entropy(ctx):
    """the shared context with the entropy leg on the device, put back afterwards"""
    ctx.set_jpeg_entropy("device")
    yield ctx
    ctx.set_jpeg_entropy("host")


def host_coefficients(name, data):
    """the yardstick, made once per file"""
    if name not in _HOST:
        count = _frame_coefficients(data)
        coef = np.zeros(count, np.int16)
        assert m.load_library().me_op_jpeg_coefficients_host(data, len(data), C.c_void_p(coef.ctypes.data), count) == 0, name
        coef.setflags(write=False)
        _HOST[name] = coef
    return _HOST[name]


def _frame_coefficients(data):
    """coefficients of all components of a frame: whole MCUs of 8 h x 8 v samples (T.81 A.2.4)"""
    at = J._sof(data)
    height, width = (data[at - 4] << 8) | data[at - 3], (data[at - 2] << 8) | data[at - 1]
    comps = [(data[at + 2 + 3 * k] >> 4, data[at + 2 + 3 * k] & 15) for k in range(data[at])]
    if len(comps) == 1:
        comps = [(1, 1)]
    hmax, vmax = max(h for h, _ in comps), max(v for _, v in comps)
    mcus = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    return sum(mcus * h * v * 64 for h, v in comps)


def entropy(ctx, name, data, bits):
    want = host_coefficients(name, data)
    got = np.full(want.size, 0x5A5A, np.int16)
    rc = ctx.lib.me_op_jpeg_entropy(ctx.handle, data, len(data), bits, C.c_void_p(got.ctypes.data), got.size)
    rep, ms = ctx.last_jpeg_entropy()
    assert rc == 0, (name, bits, rc, rep, ctx.lib.me_last_error(ctx.handle))
    assert rep["where"] == "device" and rep["reason"] == 0 and rep["subseq_bits"] == (bits or 1024), (name, rep)
    bad = int((got != want).sum())
    assert bad == 0, f"{name} at {bits} bits: {bad} of {want.size} coefficients differ"
    assert np.array_equal(got, want)
    assert rep["upload_bytes"] < 2 * len(data) + 16384 and all(v >= 0 for v in ms)    # the scan and some tables, not coefficients
    return rep


@pytest.mark.parametrize("index", range(len(SEQUENTIAL)), ids=[name for name, _ in SEQUENTIAL])
def test_coefficients_at_the_default_length(ctx, index):
    name, make = SEQUENTIAL[index]
    entropy(ctx, name, make(), 0)


@pytest.mark.parametrize("name", AT_128)
def test_coefficients_at_128_bits(ctx, name):
    entropy(ctx, name, dict(J.FILES)[name](), 128)


def test_sync_across_workgroup_seams(ctx):
    name = "517x333-s2"
    rep = entropy(ctx, name, dict(J.FILES)[name](), SMALLEST)
    assert rep["subseqs"] >= 3109 and rep["workgroups"] > 1 and rep["workgroups"] == -(-rep["subseqs"] // 256)
    assert 1 < rep["rounds"] <= 65536 // SMALLEST + 1


def test_arguments_and_declines_of_the_op(ctx):
    lib, hd = ctx.lib, ctx.handle
    data = J.plain(64, 48)
    coef = np.zeros(_frame_coefficients(data), np.int16)
    dst = C.c_void_p(coef.ctypes.data)
    for bits in (32, 100, 1 << 17):
        assert lib.me_op_jpeg_entropy(hd, data, len(data), bits, dst, coef.size) == BAD_ARG
    assert lib.me_op_jpeg_entropy(hd, data, len(data), 0, dst, coef.size - 64) == 2          # ME_ERR_BAD_SHAPE
    prog = J.plain(64, 48, 2, True, 90)
    coef[:] = 77
    assert lib.me_op_jpeg_entropy(hd, prog, len(prog), 0, dst, coef.size) == DECLINED         # no fallback inside the op
    rep, _ = ctx.last_jpeg_entropy()
    assert rep["where"] == "host" and rep["reason"] == 1 and (coef == 77).all()
    assert lib.me_ctx_set_jpeg_entropy(hd, 2) == BAD_ARG
    entropy(ctx, "64x48", data, 0)


def host(data, tmp_path, name="f", oriented=True):
    rc, want, err = J.host_decode(data, tmp_path, oriented=oriented, name=name)
    assert rc == 0, err
    return want


def check(ctx, data, want, orientation=1, where="device"):
    got = ctx.decode_jpeg(data, orientation)
    rep, _ = ctx.last_jpeg_entropy()
    assert rep["where"] == where, rep
    assert got.shape == want.shape and np.array_equal(got, want)
    return rep


def test_pixels_of_the_file_list(device_entropy, tmp_path):
    ctx = device_entropy
    for name, make in SEQUENTIAL:
        data = make()
        rep = check(ctx, data, host(data, tmp_path, name))
        assert rep["reason"] == 0, (name, rep)
    ms = ctx.last_jpeg_timing()
    assert len(ms) == 5 and all(v >= 0 for v in ms)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_pixels_of_the_orientations(device_entropy, tmp_path, orientation):
    data = J.with_exif(orientation)
    check(device_entropy, data, host(data, tmp_path), orientation)


def test_chained_resize_and_queueing(device_entropy, tmp_path):
    ctx = device_entropy
    data = J.plain(517, 333, 2, False, 90, seed=21)
    got = ctx.decode_jpeg_resized(data, (96, 96), 1)
    assert ctx.last_jpeg_entropy()[0]["where"] == "device"
    ctx.set_jpeg_entropy("host")
    assert np.array_equal(got, ctx.decode_jpeg_resized(data, (96, 96), 1))
    assert ctx.last_jpeg_entropy()[0]["where"] == "host"
    ctx.set_jpeg_entropy("device")
    # two different files queued back to back with no synchronise between the calls
    a, b = data, J.restart_rows()
    wa, wb = host(a, tmp_path, "a"), host(b, tmp_path, "b")
    oa = torch.full((333, 517, 3), 7, dtype=torch.uint8, device="cuda")
    ob = torch.full((203, 111, 3), 7, dtype=torch.uint8, device="cuda")      # b rotated: orientation 6
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.handle
    assert lib.me_jpeg_decode_rgb8(hd, a, len(a), 1, ptr(oa), 517, 333) == 0
    assert lib.me_jpeg_decode_rgb8(hd, b, len(b), 6, ptr(ob), 111, 203) == 0
    assert lib.me_ctx_synchronize(hd) == 0
    assert ctx.last_jpeg_entropy()[0]["where"] == "device"
    assert np.array_equal(oa.cpu().numpy(), wa)
    assert np.array_equal(ob.cpu().numpy(), J.orient(wb, 6))


def test_fallbacks(device_entropy, tmp_path):
    ctx = device_entropy
    lib, hd = ctx.lib, ctx.handle
    good = J.plain(64, 48)
    want = host(good, tmp_path, "good")
    prog = J.plain(203, 111, 0, True, 70, seed=22)
    rep = check(ctx, prog, host(prog, tmp_path, "prog"), where="host")
    assert rep["reason"] == 1                                                  # progressive
    check(ctx, good, want)
    for name, make, host_accepts in E.DAMAGED:
        data = make()
        rc, hwant, err = J.host_decode(data, tmp_path, name=name)
        assert (rc == 0) == host_accepts
        out = np.zeros((48, 64, 3), np.uint8)
        got = lib.me_jpeg_decode_rgb8(hd, data, len(data), 1, C.c_void_p(out.ctypes.data), 64, 48)
        if host_accepts:
            assert got == 0 and np.array_equal(out, hwant), name
        else:
            assert got == BAD_ARG
            assert err.strip().split(".jpg: ", 1)[1] == lib.me_last_error(hd).decode().split("<jpeg>: ", 1)[1]
            assert "bad Huffman code" in err
            assert ctx.last_jpeg_entropy()[0]["where"] == "host"
        check(ctx, good, want)                                                 # the context still decodes


def test_command_lines_agree(tmp_path):
    """Compiled CLI, tiny model, a 301 x 199 JPEG photo with an EXIF orientation: the depth PNG is the same file with
    MATRIX_EYES_JPEG_ENTROPY=device and =host behind MATRIX_EYES_JPEG_DECODER=device; another value is an error; the Python
    mirror writes the same depth pixels with either."""
    from PIL import Image
    from matrix_eyes_amd import reconstruction as R
    cfg = m.ModelConfig.tiny()
    ckpt = str(tmp_path / "tiny.pt")
    tiny_checkpoint(ckpt)
    src = str(tmp_path / "photo.jpg")
    exif = Image.Exif()
    exif[0x0112] = 6
    exif.get_ifd(0x8769)[0xA405] = 35
    with open(src, "wb") as f:
        f.write(J.save(J.photo(301, 199, 9), quality=90, subsampling=2, exif=exif))
    drop = ("MATRIX_EYES_RESAMPLER", "MATRIX_EYES_JPEG_DECODER", "MATRIX_EYES_JPEG_ENTROPY")
    base = {k: v for k, v in os.environ.items() if k not in drop}

    def cli(out, **extra):
        r = run_cli([CLI, f"--checkpoint-path={ckpt}", src, str(tmp_path / out)],
                    dict(base, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_JPEG_DECODER="device", **extra), expect=None, timeout=300)
        return r, ((tmp_path / out).read_bytes() if r.returncode == 0 else None)

    r, on_host = cli("depth_host.png", MATRIX_EYES_JPEG_ENTROPY="host")
    assert r.returncode == 0, r.stdout + r.stderr
    r, on_device = cli("depth_device.png", MATRIX_EYES_JPEG_ENTROPY="device")
    assert r.returncode == 0, r.stdout + r.stderr
    assert on_device == on_host and len(on_device) > 1000
    r, _ = cli("x.png", MATRIX_EYES_JPEG_ENTROPY="gpu")
    assert r.returncode != 0 and "MATRIX_EYES_JPEG_ENTROPY" in r.stdout + r.stderr      # not a silent default

    loader = m.DepthProModelLoader(ckpt, False, cfg)
    pixels = []
    for where in ("host", "device"):
        out = str(tmp_path / f"depth_py_{where}.png")
        R.extract_depth(0, loader, src, out, None, m.ImageOutputFormat.DepthMap(), m.VertexMode.Color, resampler="device",
                        jpeg_decoder="device", jpeg_entropy=where)
        assert loader.context(0, "f16").last_jpeg_entropy()[0]["where"] == where
        pixels.append(np.asarray(Image.open(out)))
    assert np.array_equal(pixels[0], pixels[1])
    assert np.array_equal(pixels[1], np.asarray(Image.open(tmp_path / "depth_device.png")))
    with pytest.raises(m.MatrixEyesError):
        R.extract_depth(0, loader, src, str(tmp_path / "y.png"), None, m.ImageOutputFormat.DepthMap(), m.VertexMode.Color,
                        jpeg_decoder="device", jpeg_entropy="gpu")
