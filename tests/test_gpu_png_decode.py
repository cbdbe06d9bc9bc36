"""GPU tests of the PNG decoder (csrc/png_decode.hip behind me_png_decode_rgb8 / me_png_decode_resized_rgb8 /
me_op_png_unfilter): byte-identical to the C++ host layer's decoder (me_op_png_decode_host: host/png_decoder.cpp from
inside the library) followed by apply_orientation, for every file of tests/png_files.py, through host and device
pointers, queued back to back, in bands of several sizes, chained with the Lanczos3 resize, and through both command
lines.  Every comparison is np.array_equal: there is no tolerance."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from util import ctx_for, ptr, run_cli, tiny_checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_files as P  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = P.ROOT
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
BAD_ARG, BAD_SHAPE = 1, 2
PLAIN = [(name, make) for name, make in P.FILES if not name.startswith("a7-")]
ADAM7 = [(name, make) for name, make in P.FILES if name.startswith("a7-")]


@pytest.fixture(scope="module")
def ctx():
    return ctx_for("tiny", "f16")         # a context is enough: no weights are loaded for a decode


def host(ctx, data, orientation=1):
    """the host decoder's pixels, then apply_orientation (restated in png_files.orient, which the CPU tests hold to
    host_selftest's)"""
    w, h, _, _ = ctx.png_info(data)
    out = np.empty((h, w, 3), np.uint8)
    rc = ctx.lib.me_op_png_decode_host(data, len(data), C.c_void_p(out.ctypes.data), w, h)
    assert rc == 0, ctx.lib.me_last_error(None)
    return np.ascontiguousarray(P.orient(out, orientation))


def check(ctx, data, want, orientation=1):
    got = ctx.decode_png(data, orientation)                                   # a host destination
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {want.size} bytes differ"
    dev = ctx.decode_png(data, orientation, out=torch.full(want.shape, 7, dtype=torch.uint8, device="cuda"))
    ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want)                             # a device destination
    return got


@pytest.mark.parametrize("index", range(len(PLAIN)), ids=[name for name, _ in PLAIN])
def test_decode_equals_the_host_decoder(ctx, index):
    name, make = PLAIN[index]
    data = make()
    o = 1 + index % 8
    check(ctx, data, host(ctx, data, o), o)


def test_adam7_with_empty_passes(ctx):
    for k, (name, make) in enumerate(ADAM7):
        data = make()
        o = 1 + k % 8
        got = ctx.decode_png(data, o)
        assert np.array_equal(got, host(ctx, data, o)), name


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientations(ctx, orientation):
    data = dict(P.FILES)[f"exif{orientation}"]()
    w, h, off, n = ctx.png_info(data)
    assert (w, h) == (13, 5) and data[off:off + 2] == b"II" and n == len(P.exif_block(orientation, 35))
    want = host(ctx, data, orientation)
    assert want.shape == ((13, 5, 3) if orientation >= 5 else (5, 13, 3))
    check(ctx, data, want, orientation)
    for name in ("t3d2i1", "t0d16i0", "tile+1px"):                             # odd widths, sub-byte pixels, two tiles
        other = dict(P.FILES)[name]()
        check(ctx, other, host(ctx, other, orientation), orientation)


def test_queued_back_to_back(ctx):
    """Two different files queued on the stream with no synchronise between them -- the second call's stream (pinned
    staging, device scratch) must not reach the first call's kernels -- then the first again on the grown scratch."""
    files = dict(P.FILES)
    a, b = files["tiles"](), files["rgba16-cycle-i"]()
    wa, wb = host(ctx, a), host(ctx, b, 6)
    oa = torch.full(wa.shape, 7, dtype=torch.uint8, device="cuda")
    ob = torch.full(wb.shape, 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.handle
    assert lib.me_png_decode_rgb8(hd, a, len(a), 1, ptr(oa), wa.shape[1], wa.shape[0]) == 0
    assert lib.me_png_decode_rgb8(hd, b, len(b), 6, ptr(ob), wb.shape[1], wb.shape[0]) == 0
    assert lib.me_ctx_synchronize(hd) == 0
    assert np.array_equal(oa.cpu().numpy(), wa)
    assert np.array_equal(ob.cpu().numpy(), wb)
    check(ctx, a, wa)
    ms = ctx.last_png_timing()
    assert len(ms) == 5 and all(v >= 0 for v in ms) and ms[4] == 0             # the last decode had a device destination
    ctx.decode_png(a)
    assert ctx.last_png_timing()[4] > 0
    # an unaligned device destination: nothing written around it
    small = files["t2d8i1"]()
    ws = host(ctx, small)
    flat = torch.full((ws.size + 8,), 77, dtype=torch.uint8, device="cuda")
    assert lib.me_png_decode_rgb8(hd, small, len(small), 1, C.c_void_p(flat.data_ptr() + 3), 33, 17) == 0
    ctx.synchronize()
    out = flat.cpu().numpy()
    assert np.array_equal(out[3:3 + ws.size].reshape(ws.shape), ws)
    assert (out[:3] == 77).all() and (out[3 + ws.size:] == 77).all()


def _stream_of(data):
    """(filtered stream, IHDR fields) of a generated file"""
    w, h, depth, ctype, _, _, il = struct.unpack(">IIBBBBB", data[16:29])
    z, pos = b"", 8
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        if data[pos + 4:pos + 8] == b"IDAT":
            z += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return np.frombuffer(zlib.decompress(z), np.uint8), (w, h, depth, ctype, il)


def _unfiltered_reference(stream, fields):
    """the reconstructed stream: the generator's own rows, filter bytes kept (independent of any decoder)"""
    w, h, depth, ctype, il = fields
    ch = P.CHANNELS[ctype]
    bpp = max(1, ch * depth // 8)
    out, pos = stream.copy(), 0
    for x0, y0, dx, dy in P.passes_of(w, h, il):
        pw, ph = (w + dx - 1 - x0) // dx, (h + dy - 1 - y0) // dy
        if pw <= 0 or ph <= 0:
            continue
        stride = (pw * ch * depth + 7) // 8
        prev = np.zeros(stride, np.int32)
        for _ in range(ph):
            kind, row = int(out[pos]), out[pos + 1:pos + 1 + stride].astype(np.int32)
            for i in range(stride):
                a = row[i - bpp] if i >= bpp else 0
                c = prev[i - bpp] if i >= bpp else 0
                b = prev[i]
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = (0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[kind]
                row[i] = (row[i] + pred) & 255
            out[pos + 1:pos + 1 + stride] = row
            prev = row
            pos += stride + 1
    return out


@pytest.mark.parametrize("name", ("rows65", "rows257", "rows-i"))
def test_unfilter_in_bands(ctx, name):
    """me_op_png_unfilter with picture rows per launch of 1, 2, one fewer than, exactly and one more than a wave's row
    group, more than the four groups a workgroup holds at once, and the default"""
    stream, (w, h, depth, ctype, il) = _stream_of(dict(P.FILES)[name]())
    want = _unfiltered_reference(stream, (w, h, depth, ctype, il))
    for band_rows in (1, 2, 63, 64, 65, 300, 0):
        got = ctx.op_png_unfilter(stream, w, h, depth, ctype, il, band_rows)
        assert np.array_equal(got, want), band_rows
    dev = torch.as_tensor(stream.copy(), device="cuda")
    got = ctx.op_png_unfilter(dev, w, h, depth, ctype, il, 64, out=dev)          # in place, device pointers
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    lib, hd = ctx.lib, ctx.handle
    out = np.empty_like(stream)
    bad = stream.copy()
    bad[0] = 5
    assert lib.me_op_png_unfilter(hd, C.c_void_p(bad.ctypes.data), len(bad), w, h, depth, ctype, il, 0, C.c_void_p(out.ctypes.data)) == BAD_ARG
    assert b"bad PNG filter" in lib.me_last_error(hd)
    assert lib.me_op_png_unfilter(hd, C.c_void_p(stream.ctypes.data), len(stream) - 1, w, h, depth, ctype, il, 0,
                                  C.c_void_p(out.ctypes.data)) == BAD_SHAPE
    assert lib.me_op_png_unfilter(hd, C.c_void_p(stream.ctypes.data), len(stream), w, h, 4, 2, il, 0, C.c_void_p(out.ctypes.data)) == BAD_ARG


def photo(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([127 + 100 * np.sin(x / 17.0 + y / 29.0), 127 + 100 * np.cos(x / 11.0 - y / 23.0),
                  127 + 90 * np.sin((x + y) / 31.0)], -1) + rng.normal(0, 6, (h, w, 3)).astype(np.float32)
    return np.clip(a, 0, 255).astype(np.uint8)


def test_a_large_picture_from_the_device_encoder(ctx):
    """1600 x 1200 8-bit RGB written by me_png_encode_rgb8: five default bands of 256 rows, 23 tiles per row, and
    1.92 M pixels on a finish grid of 1024 x 256 lanes -- eight grid rounds.  The loop closes: the decoder returns the
    picture the encoder was given."""
    img = photo(1600, 1200, 5)
    data = ctx.png_encode(img)
    want = host(ctx, data)
    assert np.array_equal(want, img)
    check(ctx, data, want)
    check(ctx, data, np.ascontiguousarray(P.orient(img, 7)), 7)


def test_chained_resize(ctx):
    files = dict(P.FILES)
    for name, orientation in (("tiles", 1), ("exif6", 6), ("t3d4i1", 8)):
        data = files[name]()
        want = ctx.resize_lanczos3(host(ctx, data, orientation), (96, 64))       # host decode, apply_orientation, me_resize_lanczos3_rgb8
        got = ctx.decode_png_resized(data, (96, 64), orientation)
        assert np.array_equal(got, want), name
        dev = ctx.decode_png_resized(data, (96, 64), orientation, out=torch.empty((64, 96, 3), dtype=torch.uint8, device="cuda"))
        ctx.synchronize()
        assert np.array_equal(dev.cpu().numpy(), want)
    same = files["t2d8i0"]()
    assert np.array_equal(ctx.decode_png_resized(same, (33, 17)), host(ctx, same))       # the same size is a copy


def test_refusals_leave_the_context_usable(ctx):
    lib, hd = ctx.lib, ctx.handle
    good = dict(P.FILES)["t3d8i1"]()                                          # a palette file: the status word is in use
    want = host(ctx, good)
    out = np.zeros((17, 33, 3), np.uint8)
    dst = C.c_void_p(out.ctypes.data)
    for name, make, words in P.REFUSED:
        bad = make()
        hout = np.zeros((7, 9, 3), np.uint8)
        assert lib.me_op_png_decode_host(bad, len(bad), C.c_void_p(hout.ctypes.data), 9, 7) == -3, name
        host_words = lib.me_last_error(None).decode()
        assert words in host_words, (name, host_words)
        bw, bh = (2, 2) if name == "short-plte-edge" else (9, 7)
        bout = np.zeros((bh, bw, 3), np.uint8)
        assert lib.me_png_decode_rgb8(hd, bad, len(bad), 1, C.c_void_p(bout.ctypes.data), bw, bh) == BAD_ARG, name
        assert lib.me_last_error(hd).decode() == host_words, name             # "<png>: ..." in both
        assert lib.me_png_decode_resized_rgb8(hd, bad, len(bad), 1, dst, 8, 8) == BAD_ARG, name
        assert lib.me_last_error(hd).decode() == host_words, name
        check(ctx, good, want)                                                 # the next decode on the same context
    calls = [
        (lambda: lib.me_png_decode_rgb8(hd, None, len(good), 1, dst, 33, 17), BAD_ARG),
        (lambda: lib.me_png_decode_rgb8(hd, good, len(good), 1, None, 33, 17), BAD_ARG),
        (lambda: lib.me_png_decode_rgb8(hd, good, len(good), 0, dst, 33, 17), BAD_ARG),
        (lambda: lib.me_png_decode_rgb8(hd, good, len(good), 9, dst, 33, 17), BAD_ARG),
        (lambda: lib.me_png_decode_rgb8(hd, good, len(good), 1, dst, 17, 33), BAD_SHAPE),
        (lambda: lib.me_png_decode_rgb8(hd, good, len(good), 6, dst, 33, 17), BAD_SHAPE),      # oriented: 17 x 33
        (lambda: lib.me_png_decode_rgb8(hd, good, len(good), 1, dst, 0, 17), BAD_SHAPE),
        (lambda: lib.me_png_decode_resized_rgb8(hd, good, len(good), 1, None, 8, 8), BAD_ARG),
        (lambda: lib.me_png_decode_resized_rgb8(hd, good, len(good), 12, dst, 8, 8), BAD_ARG),
        (lambda: lib.me_png_decode_resized_rgb8(hd, good, len(good), 1, dst, 0, 8), BAD_SHAPE),
        (lambda: lib.me_png_decode_resized_rgb8(hd, good, len(good), 1, dst, 8, 1 << 20), BAD_SHAPE),
    ]
    for k, (call, code) in enumerate(calls):
        assert call() == code, k
        assert lib.me_last_error(hd)
    check(ctx, good, want)


def test_command_lines_agree(tmp_path):
    """Compiled CLI, tiny model, a 301 x 199 PNG photo with an eXIf orientation and focal length: the depth PNG and the
    vertex-coloured PLY are the same files with MATRIX_EYES_PNG_DECODER=device and =host, with either resampler; any
    other value is an error that names the variable; and the Python mirror with the device decoder and resampler writes
    the compiled CLI's depth pixels."""
    from PIL import Image
    from matrix_eyes_amd import reconstruction as R
    cfg = m.ModelConfig.tiny()
    ckpt = str(tmp_path / "tiny.pt")
    tiny_checkpoint(ckpt)
    src = str(tmp_path / "photo.png")
    px = photo(301, 199, 9).astype(np.uint16)
    with open(src, "wb") as f:
        f.write(P.make(301, 199, 2, 8, 1, P.CYCLE, px=px, exif=P.exif_block(6, 35)))
    base = {k: v for k, v in os.environ.items() if k not in ("MATRIX_EYES_RESAMPLER", "MATRIX_EYES_PNG_DECODER")}

    def cli(out, *args, **extra):
        run_cli([CLI, f"--checkpoint-path={ckpt}", *args, src, str(tmp_path / out)], dict(base, MATRIX_EYES_MODEL="tiny", **extra),
                timeout=300)
        return (tmp_path / out).read_bytes()

    depth_host = cli("depth_host.png", MATRIX_EYES_PNG_DECODER="host")
    depth_dev = cli("depth_dev.png", MATRIX_EYES_PNG_DECODER="device")
    assert depth_dev == depth_host and len(depth_dev) > 1000
    assert cli("depth_default.png") == depth_host                                        # the default is the host decoder
    depth_dev_hr = cli("depth_dev_hr.png", MATRIX_EYES_PNG_DECODER="device", MATRIX_EYES_RESAMPLER="host")
    assert depth_dev_hr == cli("depth_host_hr.png", MATRIX_EYES_PNG_DECODER="host", MATRIX_EYES_RESAMPLER="host")
    ply_host = cli("mesh_host.ply", "--mesh=vertex-colors", MATRIX_EYES_PNG_DECODER="host")
    ply_dev = cli("mesh_dev.ply", "--mesh=vertex-colors", MATRIX_EYES_PNG_DECODER="device")
    assert ply_dev == ply_host and len(ply_dev) > 1000
    r = run_cli([CLI, f"--checkpoint-path={ckpt}", src, str(tmp_path / "x.png")],
                dict(base, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_PNG_DECODER="gpu"), expect=None, timeout=300)
    assert r.returncode != 0 and "MATRIX_EYES_PNG_DECODER" in r.stdout + r.stderr          # not a silent default

    loader = m.DepthProModelLoader(ckpt, False, cfg)
    R.extract_depth(0, loader, src, str(tmp_path / "depth_py.png"), None, m.ImageOutputFormat.DepthMap(),
                    m.VertexMode.Color, resampler="device", png_decoder="device")
    cpp, py = np.asarray(Image.open(tmp_path / "depth_dev.png")), np.asarray(Image.open(tmp_path / "depth_py.png"))
    assert cpp.shape == py.shape == (301, 199, 3)                                         # rotated by the eXIf orientation
    assert np.array_equal(cpp, py)
    with pytest.raises(m.MatrixEyesError):
        m.depth_pro.resolve_png_decoder("gpu")
