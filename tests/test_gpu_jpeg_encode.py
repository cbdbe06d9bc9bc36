"""GPU tests of the JPEG encoder (me_jpeg_encode_rgb8, me_output_jpeg, me_output_depth_map_jpeg, me_output_stereogram_jpeg):
the device's file is, byte for byte, the host layer's (me_op_jpeg_encode_host), the numpy restatement's
(tests/jpeg_encode_ref.py) and, where Pillow links libjpeg-turbo, Pillow's; across workgroup seams, from host and device
pictures, deterministically, inside its buffer, chained behind the output kernels, read back by the device decoder, and
from both command lines.

One context for the module; the yardstick's files are computed once (tests/jpeg_encode_pictures.py) and shared."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_pictures as P  # noqa: E402

import matrix_eyes_amd as m  # noqa: E402
from util import run_cli, tiny_checkpoint  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
BAD_ARG, BAD_SHAPE, IO = 1, 2, 7


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0, "f16", m.ModelConfig.tiny())   # no weights: the encoder needs a context only
    yield c
    c.close()


def host_encode(lib, rgb, quality, subsampling):
    h, w = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb)
    out = np.zeros(700 + 8 * rgb.size, np.uint8)
    n = C.c_int64()
    assert lib.me_op_jpeg_encode_host(C.c_void_p(rgb.ctypes.data), w, h, quality, subsampling, C.c_void_p(out.ctypes.data),
                                      out.size, C.byref(n)) == 0
    return out[:n.value].tobytes()


def host_decode(lib, data, w, h):
    rgb = np.zeros((h, w, 3), np.uint8)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert lib.me_op_jpeg_decode_host(buf, len(data), C.c_void_p(rgb.ctypes.data), w, h) == 0
    return rgb


class _DevMem:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


# ---- byte equality ------------------------------------------------------------------------------------------------------------

def test_equals_host_encoder_and_yardstick(ctx):
    for kind, w, h, q, s in P.cases():
        rgb = P.picture(kind, w, h)
        got = ctx.jpeg_encode(rgb, q, s)
        assert got == P.reference(kind, w, h, q, s)[0], (kind, w, h, q, s)
        assert got == host_encode(ctx.lib, rgb, q, s), (kind, w, h, q, s)
        rep, _ = ctx.last_jpeg_encode()
        st = P.reference(kind, w, h, q, s)[1]
        assert rep["blocks"] == st["blocks"] and rep["stuffed"] == st["stuffed"] and rep["file_bytes"] == len(got)


def test_equals_pillow(ctx):
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow does not link libjpeg-turbo, whose integer path the encoder restates")
    for kind, w, h, q, s in [c for c in P.cases() if c[0] != "shape" or c[3] in (25, 100)]:
        rgb = P.picture(kind, w, h)
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=s, optimize=False)
        assert ctx.jpeg_encode(rgb, q, s) == buf.getvalue(), (kind, w, h, q, s)


@pytest.mark.parametrize("subsampling", [0, 2])
def test_workgroup_seams(ctx, subsampling):
    """200 x 264 noise at quality 100: more than one workgroup of every kernel, both scans included"""
    rgb = P.picture("seams")
    want, st = P.reference("seams", 0, 0, 100, subsampling)
    assert ctx.jpeg_encode(rgb, 100, subsampling) == want
    rep, ms = ctx.last_jpeg_encode()
    assert rep["blocks"] == st["blocks"] >= 825 and rep["stuffed"] == st["stuffed"] > 256
    for name in ("fdct_groups", "wave_groups", "block_scan_groups", "stuff_groups", "stuff_scan_groups"):
        assert rep[name] > 1, (name, rep)
    assert rep["scan_bits"] > 8 * (len(want) - 623 - 2 - rep["stuffed"]) - 8 and all(t >= 0 for t in ms)


# ---- input location, determinism, scratch -------------------------------------------------------------------------------------

def test_host_and_device_pictures(ctx):
    for kind, w, h, q, s in (("shape", 37, 53, 75, 2), ("shape", 17, 33, 95, 1), ("noise", 96, 136, 100, 0)):
        rgb = P.picture(kind, w, h)
        on_device = ctx.jpeg_encode(torch.from_numpy(rgb).cuda(), q, s)
        assert on_device.is_cuda and on_device.cpu().numpy().tobytes() == ctx.jpeg_encode(rgb, q, s) == P.reference(kind, w, h, q, s)[0]


def test_deterministic_and_scratch_reuse(ctx):
    big, small = P.picture("seams"), P.picture("shape", 37, 53)
    a1 = ctx.jpeg_encode(big, 100, 0)
    b1 = ctx.jpeg_encode(small, 75, 2)               # a smaller picture in between: the scratch is reused
    a2 = ctx.jpeg_encode(big, 100, 0)
    b2 = ctx.jpeg_encode(torch.from_numpy(small).cuda(), 75, 2).cpu().numpy().tobytes()
    a3 = ctx.jpeg_encode(big, 100, 0)
    assert a1 == a2 == a3 == P.reference("seams", 0, 0, 100, 0)[0]
    assert b1 == b2 == P.reference("shape", 37, 53, 75, 2)[0]


def test_buffer_bounds(ctx):
    """The file buffer holds header + twice the packed stream + 2 bytes (stuffing can double a stream).  Filled with a
    canary and reused by smaller encodes, everything behind the reported size keeps the canary."""
    lib, h = ctx.lib, ctx.handle
    ptr, n = C.c_void_p(), C.c_int64()

    def encode(rgb, q, s):
        rgb = np.ascontiguousarray(rgb)
        ctx._check(lib.me_jpeg_encode_rgb8(h, C.c_void_p(rgb.ctypes.data), rgb.shape[1], rgb.shape[0], q, s, C.byref(ptr), C.byref(n)))
        return int(ptr.value), int(n.value)

    at, size = encode(P.picture("seams"), 100, 0)
    rep, _ = ctx.last_jpeg_encode()
    capacity = rep["capacity"]
    assert size <= capacity == 623 + 2 * (size - 623 - 2 - rep["stuffed"]) + 2
    whole = torch.as_tensor(_DevMem(at, capacity), device="cuda")
    for kind, w, hh, q, s in (("noise", 96, 136, 100, 0), ("shape", 37, 53, 75, 2), ("flat", 64, 80, 75, 1), ("shape", 1, 1, 1, 0)):
        whole.fill_(0xA5)
        torch.cuda.synchronize()
        at2, size2 = encode(P.picture(kind, w, hh), q, s)
        assert at2 == at and size2 < size             # the same buffer, grown to the high-water mark only
        got = whole.cpu().numpy()
        assert got[:size2].tobytes() == P.reference(kind, w, hh, q, s)[0]
        assert (got[size2:] == 0xA5).all(), (kind, int(np.flatnonzero(got[size2:] != 0xA5)[0]))


# ---- chained calls --------------------------------------------------------------------------------------------------------------

def _field():
    yy, xx = np.mgrid[0:96, 0:96].astype(np.float32)
    return (0.02 + 0.5 * (1.0 + np.sin(xx / 11.0) * np.cos(yy / 7.0)) * (1.0 + xx / 96.0)).astype(np.float32)


@pytest.mark.parametrize("overlap", [0, 1])
def test_chained_calls(ctx, tmp_path, overlap):
    """me_output_depth_map_jpeg / me_output_stereogram_jpeg write the file the host encoder makes of the picture that
    me_depthmap_rgb_resized / me_stereogram return; from a host and from a device depth buffer"""
    field = _field()
    dm = m.DepthMap(ctx, field, (150, 112))
    rgb = dm.depth_map_rgb_resized()
    noise = P.noise(75, 56, seed=5)
    st = dm.stereogram(0.5, 1.0 / 16.0, noise)
    assert rgb.shape == (112, 150, 3) and st.shape == (56, 75, 3)
    want_depth, want_stereo = host_encode(ctx.lib, rgb, 90, 0), host_encode(ctx.lib, st, 75, 2)
    ctx.set_output_overlap(bool(overlap))
    try:
        dm.output_depth_map_jpeg(str(tmp_path / "a.jpg"), 90, 0)
        dm.output_stereogram_jpeg(str(tmp_path / "b.jpg"), 0.5, 1.0 / 16.0, noise, 75, 2)
        ctx.output_jpeg(rgb, str(tmp_path / "c.jpeg"), 90, 0)
        depth = torch.from_numpy(dm.data.copy()).cuda()
        torch.cuda.synchronize()
        mn, mx = dm.inverse_depth_range()
        ctx._check(ctx.lib.me_output_depth_map_jpeg(ctx.handle, C.c_void_p(depth.data_ptr()), 96, 96, mn, mx, None, 150, 112, 90, 0,
                                                    str(tmp_path / "d.jpg").encode()))
        nz = torch.from_numpy(noise).cuda()
        torch.cuda.synchronize()
        ctx._check(ctx.lib.me_output_stereogram_jpeg(ctx.handle, C.c_void_p(depth.data_ptr()), 96, 96, mn, mx, 75, 56, 1.0 / 16.0,
                                                     C.c_void_p(nz.data_ptr()), 75, 2, str(tmp_path / "e.jpg").encode()))
        rep, ms = ctx.last_jpeg_encode()
        assert rep["file_bytes"] == len(want_stereo) and ms[5] > 0
    finally:
        ctx.set_output_overlap(False)
    assert (tmp_path / "a.jpg").read_bytes() == (tmp_path / "c.jpeg").read_bytes() == (tmp_path / "d.jpg").read_bytes() == want_depth
    assert (tmp_path / "b.jpg").read_bytes() == (tmp_path / "e.jpg").read_bytes() == want_stereo
    # DepthMap.output_image with the encoder named: the device's file is Pillow's
    fmt = m.ImageOutputFormat.DepthMap()
    for name, enc in (("f.jpg", "device"), ("g.jpg", "pillow")):
        dm.output_image(str(tmp_path / name), "", fmt, m.VertexMode.Color, resampler="device", jpeg_encoder=enc, jpeg_quality=90,
                        jpeg_subsampling="4:4:4")
    assert (tmp_path / "f.jpg").read_bytes() == want_depth
    from PIL import features
    if features.check_feature("libjpeg_turbo"):
        assert (tmp_path / "g.jpg").read_bytes() == want_depth


# ---- the project's own decoder closes the loop ------------------------------------------------------------------------------------

def test_round_trip_on_the_device(ctx, tmp_path):
    """The files the output calls write (depth map, stereogram, a plain picture) and every file of the byte-equality test go
    through me_jpeg_decode_rgb8 with the device entropy decoder: single-scan baseline files, not declined, the host decoder's
    pixels.

    The pictures of uniform noise at quality 100 (`noise`, the seam picture) are held to the pixels only.  Every block of
    such a file carries 63 non-zero AC coefficients and no EOB, so a decoder that started at a wrong bit finds the right
    bit soon but keeps a wrong zigzag index and block number for as long as no EOB or table change re-aligns them; the
    entropy decoder synchronises on (bit, block, index), gives up after 65536 bits as its contract says (reason 12) and the
    host loop decodes the file.  Measured on an MI355X: `noise` 4:4:4 decoded on the device, `noise` 4:2:2 and the seam
    picture 4:2:0 declined after 65 rounds.  These are libjpeg's own bytes (the files equal Pillow's), so the decline is a
    property of that decoder on such streams, not of the encoder; it is printed, and anything but reason 12 fails."""
    def check(data, w, h, must_stay, what):
        got = ctx.decode_jpeg(data)
        rep, _ = ctx.last_jpeg_entropy()
        if must_stay:
            assert rep["where"] == "device" and rep["reason"] == 0, (what, rep)
        else:
            print(f"{what}: entropy decoded on the {rep['where']}, reason {rep['reason']}, rounds {rep['rounds']}")
            assert rep["reason"] in (0, 12), (what, rep)
        assert np.array_equal(got, host_decode(ctx.lib, data, w, h)), what

    ctx.set_jpeg_entropy("device")
    try:
        dm = m.DepthMap(ctx, _field(), (150, 112))
        dm.output_depth_map_jpeg(str(tmp_path / "a.jpg"), 90, 0)
        dm.output_stereogram_jpeg(str(tmp_path / "b.jpg"), 0.5, 1.0 / 16.0, P.noise(75, 56, seed=5), 75, 2)
        ctx.output_jpeg(P.picture("shape", 37, 53), str(tmp_path / "c.jpg"), 75, 1)
        for name, w, h in (("a.jpg", 150, 112), ("b.jpg", 75, 56), ("c.jpg", 37, 53)):
            check((tmp_path / name).read_bytes(), w, h, True, name)
        for kind, w, h, q, s in P.cases():
            check(P.reference(kind, w, h, q, s)[0], w, h, kind != "noise", (kind, w, h, q, s))
        for s in (0, 2):
            check(ctx.jpeg_encode(P.picture("seams"), 100, s), P.SEAMS[0], P.SEAMS[1], False, ("seams", s))
    finally:
        ctx.set_jpeg_entropy("host")


# ---- both command lines ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["compiled", "python"])
def test_command_lines(tmp_path, which):
    """MATRIX_EYES_JPEG_ENCODER=device writes the file the default (host / Pillow) writes, for the depth picture and the
    stereogram; a bad value of any of the three variables is an error and writes nothing"""
    from PIL import Image, features
    from matrix_eyes_amd.synthetic import synthetic_images
    assert os.path.exists(CLI), "the compiled command line is built by __graft_entry__.build()"
    turbo = features.check_feature("libjpeg_turbo")
    S = m.ModelConfig.tiny().img_size
    ckpt, src = str(tmp_path / "tiny.pt"), str(tmp_path / "photo.png")
    tiny_checkpoint(ckpt)
    Image.fromarray(synthetic_images(1, S, "structured", seed=11)[0]).resize((S + 88, S - 40)).save(src)
    argv = [CLI] if which == "compiled" else [sys.executable, "-m", "matrix_eyes_amd"]
    base = dict(os.environ, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_SEED="7", PYTHONPATH=ROOT)
    for name in ("MATRIX_EYES_JPEG_ENCODER", "MATRIX_EYES_JPEG_QUALITY", "MATRIX_EYES_JPEG_SUBSAMPLING"):
        base.pop(name, None)

    def run(env, *args, expect=0):
        return run_cli(argv + [f"--checkpoint-path={ckpt}", "--focal-length=35", *args], env, expect)

    dev = dict(base, MATRIX_EYES_JPEG_ENCODER="device")
    for name, flags, extra in (("depth", [], {}),
                               ("stereo", ["--image-output-format=stereogram"],
                                {"MATRIX_EYES_JPEG_QUALITY": "90", "MATRIX_EYES_JPEG_SUBSAMPLING": "4:4:4"})):
        plain, device = str(tmp_path / f"{name}_plain.jpg"), str(tmp_path / f"{name}_device.JPEG")
        run(dict(base, **extra), *flags, src, plain)
        run(dict(dev, **extra), *flags, src, device)
        data = open(device, "rb").read()
        if which == "compiled" or turbo:                      # the Python mirror's default is Pillow: libjpeg-turbo's bytes
            assert data == open(plain, "rb").read()
        assert len(data) > 2000
        img = Image.open(io.BytesIO(data))
        assert img.size == (S + 88, S - 40) and img.mode == "RGB"
        assert (b"\xff\xc0\x00\x11\x08" in data) and data[data.index(b"\xff\xc0") + 11] == (0x11 if extra else 0x22)
    for name, value in (("MATRIX_EYES_JPEG_ENCODER", "fpga"), ("MATRIX_EYES_JPEG_QUALITY", "0")):
        r = run(dict(base, **{name: value}), src, str(tmp_path / "x.jpg"), expect=1 if which == "compiled" else 2)
        assert name in r.stdout + r.stderr and not (tmp_path / "x.jpg").exists()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_errors(ctx, tmp_path):
    lib, h = ctx.lib, ctx.handle
    rgb = P.picture("shape", 16, 16)
    p = C.c_void_p(rgb.ctypes.data)
    ptr, n = C.c_void_p(), C.c_int64()
    good = str(tmp_path / "ok.jpg").encode()
    assert lib.me_jpeg_encode_rgb8(h, None, 16, 16, 75, 2, C.byref(ptr), C.byref(n)) == BAD_ARG
    assert lib.me_jpeg_encode_rgb8(h, p, 16, 16, 75, 2, None, C.byref(n)) == BAD_ARG
    assert lib.me_jpeg_encode_rgb8(h, p, 16, 16, 75, 2, C.byref(ptr), None) == BAD_ARG
    assert lib.me_output_jpeg(h, None, 16, 16, 75, 2, good) == BAD_ARG and lib.me_output_jpeg(h, p, 16, 16, 75, 2, None) == BAD_ARG
    for q, s in ((0, 2), (101, 2), (-5, 0), (75, 3), (75, -1)):
        assert lib.me_jpeg_encode_rgb8(h, p, 16, 16, q, s, C.byref(ptr), C.byref(n)) == BAD_ARG, (q, s)
        assert lib.me_output_jpeg(h, p, 16, 16, q, s, good) == BAD_ARG, (q, s)
    for w, hh in ((0, 16), (16, 0), (-1, 16), (16385, 16), (16, 16385), (65536, 1)):
        assert lib.me_jpeg_encode_rgb8(h, p, w, hh, 75, 2, C.byref(ptr), C.byref(n)) == BAD_SHAPE, (w, hh)
        assert lib.me_output_jpeg(h, p, w, hh, 75, 2, good) == BAD_SHAPE, (w, hh)
    assert not os.path.exists(good)
    assert lib.me_output_jpeg(h, p, 16, 16, 75, 2, str(tmp_path / "no" / "such" / "dir.jpg").encode()) == IO
    assert "cannot create" in lib.me_last_error(h).decode()
    depth = np.full((8, 8), 0.5, np.float32)
    pd = C.c_void_p(depth.ctypes.data)
    noise = P.noise(8, 8)
    pn = C.c_void_p(noise.ctypes.data)
    assert lib.me_output_depth_map_jpeg(h, None, 8, 8, 0.1, 1.0, None, 8, 8, 75, 2, good) == BAD_ARG
    assert lib.me_output_depth_map_jpeg(h, pd, 8, 8, 0.1, 1.0, None, 8, 8, 101, 2, good) == BAD_ARG
    assert lib.me_output_depth_map_jpeg(h, pd, 8, 8, 0.1, 1.0, None, 0, 8, 75, 2, good) == BAD_SHAPE
    assert lib.me_output_depth_map_jpeg(h, pd, 8, 8, 0.1, 1.0, None, 8, 8, 75, 2, str(tmp_path / "no" / "d.jpg").encode()) == IO
    assert lib.me_output_stereogram_jpeg(h, pd, 8, 8, 0.1, 1.0, 8, 8, 0.0625, None, 75, 2, good) == BAD_ARG
    assert lib.me_output_stereogram_jpeg(h, pd, 8, 8, 0.1, 1.0, 8, 8, 0.0625, pn, 75, 5, good) == BAD_ARG
    assert lib.me_output_stereogram_jpeg(h, pd, 8, 8, 0.1, 1.0, 8, 16385, 0.0625, pn, 75, 2, good) == BAD_SHAPE
    assert lib.me_output_stereogram_jpeg(h, pd, 8, 8, 0.1, 1.0, 8, 8, 0.0625, pn, 75, 2, str(tmp_path / "no" / "s.jpg").encode()) == IO
    # wrong in two ways: the quality is checked before the picture's size, the depth's rows and columns before either; and no
    # entry touches a missing context
    assert lib.me_output_jpeg(h, p, 0, 8, 0, 2, good) == BAD_ARG
    assert lib.me_output_depth_map_jpeg(h, pd, 8, 8, 0.1, 1.0, None, 0, 8, 101, 2, good) == BAD_ARG
    assert lib.me_output_stereogram_jpeg(h, pd, 0, 8, 0.1, 1.0, 8, 8, 0.0625, pn, 101, 2, good) == BAD_SHAPE
    assert lib.me_output_stereogram_jpeg(h, pd, 8, 8, 0.1, 1.0, 8, 16385, 0.0625, pn, 101, 2, good) == BAD_ARG
    assert lib.me_output_jpeg(None, p, 8, 8, 75, 2, good) == BAD_ARG
    assert lib.me_output_depth_map_jpeg(None, pd, 8, 8, 0.1, 1.0, None, 8, 8, 75, 2, good) == BAD_ARG
    assert lib.me_output_stereogram_jpeg(None, pd, 8, 8, 0.1, 1.0, 8, 8, 0.0625, pn, 75, 2, good) == BAD_ARG
    assert not os.path.exists(good)
    assert lib.me_last_jpeg_encode(h, None, None) == BAD_ARG
    # the context still encodes
    assert ctx.jpeg_encode(rgb, 75, 2) == P.reference("shape", 16, 16, 75, 2)[0]
