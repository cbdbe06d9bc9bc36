"""GPU tests of the JPEG decoder (csrc/jpeg_decode.hip behind me_jpeg_decode_rgb8 / me_jpeg_decode_resized_rgb8): byte-identical
to the C++ host layer's decoder followed by apply_orientation -- `host_selftest decode <in> <out.ppm> oriented` -- for every
file of tests/jpeg_files.py, through host and device pointers, queued back to back, chained with the Lanczos3 resize, and
through both command lines.  Every comparison is np.array_equal: there is no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from oracle import output_oracle as OO
from util import ctx_for, ptr, run_cli, tiny_checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_files as J  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = J.ROOT
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
_ORACLE = None
BAD_ARG, BAD_SHAPE = 1, 2


@pytest.fixture(scope="module")
def ctx():
    return ctx_for("tiny", "f16")         # a context is enough: no weights are loaded for a decode


def host(data, tmp_path, name="f", oriented=True):
    rc, want, err = J.host_decode(data, tmp_path, oriented=oriented, name=name)
    assert rc == 0, err
    return want


def check(ctx, data, want, orientation=1):
    got = ctx.decode_jpeg(data, orientation)                                  # a host destination
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {want.size} bytes differ"
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("index", range(len(J.FILES)), ids=[name for name, _ in J.FILES])
def test_decode_equals_the_host_decoder(ctx, tmp_path, index):
    name, make = J.FILES[index]
    data = make()
    check(ctx, data, host(data, tmp_path))


def test_more_than_one_grid_round(ctx, tmp_path):
    """jpeg_idct_kernel takes 32 blocks per workgroup and grid round (4 waves x 8 blocks) on at most 1024 workgroups (4 on
    each of 256 CUs): one round covers 32768 blocks.  1600 x 1200 at 4:2:0 is 100 x 75 MCUs of 6 blocks = 45000 blocks, so
    383 workgroups go round a second time (and (517, 333) above, 33 x 21 x 6 = 4158 blocks, is 130 workgroups)."""
    data = J.plain(1600, 1200, 2, False, 90, seed=5)
    want = host(data, tmp_path)
    assert want.shape == (1200, 1600, 3)
    check(ctx, data, want)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientations(ctx, tmp_path, orientation):
    """through the argument, on the file whose EXIF block says the same -- which the oracle applies"""
    data = J.with_exif(orientation)
    want = host(data, tmp_path)                                               # decode + apply_orientation(EXIF value)
    assert want.shape == ((123, 77, 3) if orientation >= 5 else (77, 123, 3))
    w, h, off, n = ctx.jpeg_info(data)
    assert (w, h) == (123, 77) and n > 0 and data[off:off + 2] in (b"II", b"MM")
    from PIL import Image
    import io
    assert Image.open(io.BytesIO(data)).getexif()[0x0112] == orientation      # what a caller reads from that block
    check(ctx, data, want, orientation)
    # and on a file without EXIF: the same pixels, remapped
    plain = J.plain(123, 77, 2, False, 90, seed=3)
    check(ctx, plain, J.orient(host(plain, tmp_path, "plain"), orientation), orientation)
    # a 4:4:4 picture whose width leaves the dword path (3 * 4 pixels) with a ragged tail and odd row starts
    odd = J.plain(37, 21, 0, False, 90, seed=4)
    check(ctx, odd, J.orient(host(odd, tmp_path, "odd"), orientation), orientation)


def test_host_and_device_destinations_and_queueing(ctx, tmp_path):
    """Two different files queued back to back on the stream with no synchronise between them -- the second call's
    coefficients (pinned staging, device scratch), planes and tables must not reach the first call's kernels -- then the
    first file again on the grown scratch."""
    a, b = J.plain(517, 333, 2, False, 90, seed=21), J.plain(203, 111, 0, True, 70, seed=22)
    wa, wb = host(a, tmp_path, "a"), host(b, tmp_path, "b")
    oa = torch.full((333, 517, 3), 7, dtype=torch.uint8, device="cuda")
    ob = torch.full((203, 111, 3), 7, dtype=torch.uint8, device="cuda")      # b rotated: orientation 6
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.handle
    assert lib.me_jpeg_decode_rgb8(hd, a, len(a), 1, ptr(oa), 517, 333) == 0
    assert lib.me_jpeg_decode_rgb8(hd, b, len(b), 6, ptr(ob), 111, 203) == 0
    assert lib.me_ctx_synchronize(hd) == 0
    assert np.array_equal(oa.cpu().numpy(), wa)
    assert np.array_equal(ob.cpu().numpy(), J.orient(wb, 6))
    check(ctx, a, wa)                                                          # host destination, scratch reused
    dev = ctx.decode_jpeg(a, 1, out=torch.empty((333, 517, 3), dtype=torch.uint8, device="cuda"))
    ctx.synchronize()
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), wa)
    # an unaligned device destination: the byte path of the stores, nothing written around it
    small = J.plain(64, 48, 2, False, 90, seed=3)
    ws = host(small, tmp_path, "s")
    flat = torch.full((64 * 48 * 3 + 8,), 77, dtype=torch.uint8, device="cuda")
    assert lib.me_jpeg_decode_rgb8(hd, small, len(small), 1, C.c_void_p(flat.data_ptr() + 3), 64, 48) == 0
    ctx.synchronize()
    out = flat.cpu().numpy()
    assert np.array_equal(out[3:3 + ws.size].reshape(ws.shape), ws)
    assert (out[:3] == 77).all() and (out[3 + ws.size:] == 77).all()
    ms = ctx.last_jpeg_timing()
    assert len(ms) == 5 and all(v >= 0 for v in ms) and ms[4] == 0             # the last decode had a device destination


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


def test_chained_resize(ctx, tmp_path):
    for name, data, orientation in (("big", J.plain(517, 333, 2, False, 90, seed=21), 1), ("exif", J.with_exif(6), 6)):
        got = ctx.decode_jpeg_resized(data, (96, 96), orientation)
        assert np.array_equal(got, ctx.resize_lanczos3(ctx.decode_jpeg(data, orientation), (96, 96)))
        assert np.array_equal(got, oracle_resize(host(data, tmp_path, name), 96, 96))   # the image oracle on the host decode
        dev = ctx.decode_jpeg_resized(data, (96, 96), orientation, out=torch.empty((96, 96, 3), dtype=torch.uint8, device="cuda"))
        ctx.synchronize()
        assert np.array_equal(dev.cpu().numpy(), got)
    same = J.plain(64, 48, 1, False, 90)
    assert np.array_equal(ctx.decode_jpeg_resized(same, (64, 48)), host(same, tmp_path, "same"))     # the same size is a copy


def test_refusals_leave_the_context_usable(ctx, tmp_path):
    lib, hd = ctx.lib, ctx.handle
    good = J.plain(64, 48)
    want = host(good, tmp_path, "good")
    out = np.zeros((48, 64, 3), np.uint8)
    dst = C.c_void_p(out.ctypes.data)
    cmyk = J.cmyk()
    assert lib.me_jpeg_decode_rgb8(hd, cmyk, len(cmyk), 1, dst, 32, 32) == BAD_ARG
    assert b"4 components" in lib.me_last_error(hd)
    assert lib.me_jpeg_decode_resized_rgb8(hd, cmyk, len(cmyk), 1, dst, 64, 48) == BAD_ARG
    assert b"4 components" in lib.me_last_error(hd)
    check(ctx, good, want)
    # the one truncation: the host decoder's bytes, or its refusal -- never a fault
    trunc = J.plain(123, 77)[:300]
    rc, twant, err = J.host_decode(trunc, tmp_path, name="trunc")
    tout = np.zeros((77, 123, 3), np.uint8)
    got = lib.me_jpeg_decode_rgb8(hd, trunc, len(trunc), 1, C.c_void_p(tout.ctypes.data), 123, 77)
    if rc == 0:
        assert got == 0 and np.array_equal(tout, twant)
    else:
        assert got == BAD_ARG
        assert err.strip().split(".jpg: ", 1)[1] == lib.me_last_error(hd).decode().split("<jpeg>: ", 1)[1]
    check(ctx, good, want)
    calls = [
        (lambda: lib.me_jpeg_decode_rgb8(hd, None, len(good), 1, dst, 64, 48), BAD_ARG),
        (lambda: lib.me_jpeg_decode_rgb8(hd, good, len(good), 1, None, 64, 48), BAD_ARG),
        (lambda: lib.me_jpeg_decode_rgb8(hd, good, len(good), 0, dst, 64, 48), BAD_ARG),
        (lambda: lib.me_jpeg_decode_rgb8(hd, good, len(good), 9, dst, 64, 48), BAD_ARG),
        (lambda: lib.me_jpeg_decode_rgb8(hd, good, len(good), 1, dst, 48, 64), BAD_SHAPE),
        (lambda: lib.me_jpeg_decode_rgb8(hd, good, len(good), 6, dst, 64, 48), BAD_SHAPE),      # oriented: 48 x 64
        (lambda: lib.me_jpeg_decode_rgb8(hd, good, len(good), 1, dst, 0, 48), BAD_SHAPE),
        (lambda: lib.me_jpeg_decode_resized_rgb8(hd, good, len(good), 1, None, 8, 8), BAD_ARG),
        (lambda: lib.me_jpeg_decode_resized_rgb8(hd, good, len(good), 12, dst, 8, 8), BAD_ARG),
        (lambda: lib.me_jpeg_decode_resized_rgb8(hd, good, len(good), 1, dst, 0, 8), BAD_SHAPE),
        (lambda: lib.me_jpeg_decode_resized_rgb8(hd, good, len(good), 1, dst, 8, 1 << 20), BAD_SHAPE),
    ]
    for k, (call, code) in enumerate(calls):
        assert call() == code, k
        assert lib.me_last_error(hd)
        check(ctx, good, want)
    with pytest.raises(m.MatrixEyesError):
        m.depth_pro.resolve_jpeg_decoder("gpu")


def test_command_lines_agree(tmp_path):
    """Compiled CLI, tiny model, a 301 x 199 JPEG photo with an EXIF orientation: the depth PNG and the vertex-coloured PLY are
    the same files with MATRIX_EYES_JPEG_DECODER=device and =host, with either resampler; and the Python mirror with the
    device decoder and resampler writes the same depth pixels."""
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
    base = {k: v for k, v in os.environ.items() if k not in ("MATRIX_EYES_RESAMPLER", "MATRIX_EYES_JPEG_DECODER")}

    def cli(out, *args, **extra):
        run_cli([CLI, f"--checkpoint-path={ckpt}", *args, src, str(tmp_path / out)], dict(base, MATRIX_EYES_MODEL="tiny", **extra),
                timeout=300)
        return (tmp_path / out).read_bytes()

    depth_host = cli("depth_host.png", MATRIX_EYES_JPEG_DECODER="host")
    depth_dev = cli("depth_dev.png", MATRIX_EYES_JPEG_DECODER="device")
    assert depth_dev == depth_host and len(depth_dev) > 1000
    assert cli("depth_default.png") == depth_host                                        # the default is the host decoder
    depth_dev_hr = cli("depth_dev_hr.png", MATRIX_EYES_JPEG_DECODER="device", MATRIX_EYES_RESAMPLER="host")
    assert depth_dev_hr == depth_host                                                    # me_jpeg_decode_rgb8 into a host RgbImage
    ply_host = cli("mesh_host.ply", "--mesh=vertex-colors", MATRIX_EYES_JPEG_DECODER="host")
    ply_dev = cli("mesh_dev.ply", "--mesh=vertex-colors", MATRIX_EYES_JPEG_DECODER="device")
    assert ply_dev == ply_host and len(ply_dev) > 1000
    r = run_cli([CLI, f"--checkpoint-path={ckpt}", src, str(tmp_path / "x.png")],
                dict(base, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_JPEG_DECODER="gpu"), expect=None, timeout=300)
    assert r.returncode != 0 and "MATRIX_EYES_JPEG_DECODER" in r.stdout + r.stderr        # not a silent default

    loader = m.DepthProModelLoader(ckpt, False, cfg)
    R.extract_depth(0, loader, src, str(tmp_path / "depth_py.png"), None, m.ImageOutputFormat.DepthMap(),
                    m.VertexMode.Color, resampler="device", jpeg_decoder="device")
    cpp, py = np.asarray(Image.open(tmp_path / "depth_dev.png")), np.asarray(Image.open(tmp_path / "depth_py.png"))
    assert cpp.shape == py.shape == (301, 199, 3)                                         # rotated by the EXIF orientation
    assert np.array_equal(cpp, py)
