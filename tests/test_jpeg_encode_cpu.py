"""CPU tests of the JPEG encoder.  The yardstick first: tests/jpeg_encode_ref.py, the numpy restatement of libjpeg's baseline
path, equals Pillow (libjpeg-turbo) byte for byte.  Then the same inputs through three encoders that must give its bytes:
csrc/jpeg_encode.h run lane by lane in the kernels' order (tests/jpeg_encode_host.cpp, plain and under the address and
undefined-behaviour sanitizers) and the host layer's sequential encode_jpeg (me_op_jpeg_encode_host).  The three named
pictures carry the conditions they are there for, every file decodes with the project's decoder and with Pillow, the new
entry points reject a null context, and the switches of both command lines are checked."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_encode_pictures as P  # noqa: E402
import jpeg_encode_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "matrix-eyes_amd")
SELFTEST = os.path.join(PKG, "host_selftest")
SOURCE = os.path.join(ROOT, "tests", "jpeg_encode_host.cpp")


def _build(exe, *extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-o", exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.exists(SELFTEST)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("jpeg_encode") / "jpeg_encode_host"))


@pytest.fixture(scope="module")
def twin_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("jpeg_encode_san") / "jpeg_encode_host_san"),
                  "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run_twin(exe, rgb, quality, subsampling, tmp_path):
    """(file bytes, report dict) of the lane-by-lane twin"""
    src, dst = str(tmp_path / "in.rgb"), str(tmp_path / "out.jpg")
    rgb.tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    h, w = rgb.shape[:2]
    r = subprocess.run([exe, src, str(w), str(h), str(quality), str(subsampling), dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rep = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    with open(dst, "rb") as f:
        return f.read(), rep


def host_encode(lib, rgb, quality, subsampling):
    h, w = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb)
    out = np.zeros(700 + 8 * rgb.size, np.uint8)
    n = C.c_int64()
    rc = lib.me_op_jpeg_encode_host(C.c_void_p(rgb.ctypes.data), w, h, quality, subsampling, C.c_void_p(out.ctypes.data), out.size,
                                    C.byref(n))
    assert rc == 0, rc
    return out[:n.value].tobytes()


def test_yardstick_equals_pillow():
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("THE YARDSTICK IS UNCHECKED: this Pillow does not link libjpeg-turbo, whose integer path the rules restate")
    for kind, w, h, q, s in P.cases():
        buf = io.BytesIO()
        Image.fromarray(P.picture(kind, w, h)).save(buf, "JPEG", quality=q, subsampling=s, optimize=False)
        assert P.reference(kind, w, h, q, s)[0] == buf.getvalue(), (kind, w, h, q, s)
    # Pillow's save defaults are quality 75, 4:2:0: what both command lines write when nothing is set
    buf = io.BytesIO()
    Image.fromarray(P.picture("shape", 37, 53)).save(buf, "JPEG")
    assert P.reference("shape", 37, 53, 75, 2)[0] == buf.getvalue()


def test_header_layout():
    data = P.reference("shape", 37, 53, 75, 2)[0]
    assert data[:4] == b"\xff\xd8\xff\xe0" and data[-2:] == b"\xff\xd9"
    head = R.header(37, 53, 75, 2, 2)
    assert len(head) == 623 and data.startswith(head)
    assert head.count(b"\xff\xdb\x00\x43") == 2 and head.count(b"\xff\xc4") == 4 and b"\xff\xc4\x00\xb5\x10" in head
    assert b"\xff\xc0\x00\x11\x08\x00\x35\x00\x25\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01" in head
    assert head.endswith(b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00") and b"\xff\xdd" not in head


def test_named_pictures_meet_their_conditions():
    for s in P.SUBSAMPLINGS:
        st = P.reference("checker", 40, 72, 10, s)[1]
        assert st["longest_run"] >= 48 and st["zrl"] >= 1, st
        st = P.reference("noise", 96, 136, 100, s)[1]
        assert st["stuffed"] >= 100, st
        data, st = P.reference("flat", 64, 80, 75, s)
        assert (len(data) - 623 - 2) * 8 < 8 * st["blocks"], st          # under 8 bits a block: blocks share output words
    st = P.reference("shape", 37, 53, 75, 2)[1]
    assert st["dummy_blocks"] == 6 * 8 - 5 * 7 and st["blocks"] == 3 * 4 * 6      # right column, bottom row and the corner MCU


def _twin_equals_the_yardstick(exe, tmp_path):
    for kind, w, h, q, s in P.cases():
        want, st = P.reference(kind, w, h, q, s)
        got, rep = run_twin(exe, P.picture(kind, w, h), q, s, tmp_path)
        assert got == want, (kind, w, h, q, s)
        assert rep["blocks"] == st["blocks"] and rep["stuffed"] == st["stuffed"] and rep["bytes"] == len(want)


def test_twin_equals_the_yardstick(twin, tmp_path):
    _twin_equals_the_yardstick(twin, tmp_path)


def test_twin_equals_the_yardstick_under_sanitizers(twin_san, tmp_path):
    _twin_equals_the_yardstick(twin_san, tmp_path)


def test_twin_on_the_seam_picture_under_sanitizers(twin_san, tmp_path):
    """the picture the GPU test crosses workgroup seams with, through buffers of exactly the device path's sizes"""
    for s in (0, 2):
        want, st = P.reference("seams", 0, 0, 100, s)
        got, rep = run_twin(twin_san, P.picture("seams"), 100, s, tmp_path)
        assert got == want and rep["blocks"] >= 825 and rep["stuffed"] == st["stuffed"] > 256


def test_host_encoder_equals_the_yardstick(lib):
    for kind, w, h, q, s in P.cases():
        assert host_encode(lib, P.picture(kind, w, h), q, s) == P.reference(kind, w, h, q, s)[0], (kind, w, h, q, s)
    assert host_encode(lib, P.picture("seams"), 100, 2) == P.reference("seams", 0, 0, 100, 2)[0]


def test_host_encoder_refusals(lib):
    rgb = P.picture("shape", 8, 8)
    out = np.zeros(4096, np.uint8)
    n = C.c_int64()
    po, pr = C.c_void_p(out.ctypes.data), C.c_void_p(rgb.ctypes.data)
    assert lib.me_op_jpeg_encode_host(None, 8, 8, 75, 2, po, out.size, C.byref(n)) == -1
    assert lib.me_op_jpeg_encode_host(pr, 8, 8, 75, 2, po, out.size, None) == -1
    for bad in ((0, 8, 75, 2), (8, -1, 75, 2), (8, 8, 0, 2), (8, 8, 101, 2), (8, 8, 75, 3), (8, 8, 75, -1)):
        assert lib.me_op_jpeg_encode_host(pr, *bad, po, out.size, C.byref(n)) == -2, bad
    assert lib.me_op_jpeg_encode_host(pr, 8, 8, 75, 2, po, 100, C.byref(n)) == -3 and n.value > 623
    assert not out.any()


def test_files_decode_with_both_decoders(lib):
    """the project's decode_jpeg (me_op_jpeg_decode_host) and Pillow read every file, to the same size"""
    from PIL import Image
    for kind, w, h, q, s in P.cases():
        data = P.reference(kind, w, h, q, s)[0]
        img = Image.open(io.BytesIO(data))
        img.load()
        assert img.size == (w, h) and img.mode == "RGB"
        rgb = np.zeros((h, w, 3), np.uint8)
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        assert lib.me_op_jpeg_decode_host(buf, len(data), C.c_void_p(rgb.ctypes.data), w, h) == 0, (kind, w, h, q, s)
        if q >= 95 and kind != "noise":
            assert np.abs(rgb.astype(int) - np.asarray(img).astype(int)).max() <= 16


def test_null_context_is_rejected(lib):
    rgb = P.picture("shape", 8, 8)
    p = C.c_void_p(rgb.ctypes.data)
    ptr, n = C.c_void_p(), C.c_int64()
    assert lib.me_jpeg_encode_rgb8(None, p, 8, 8, 75, 2, C.byref(ptr), C.byref(n)) == 1
    assert lib.me_output_jpeg(None, p, 8, 8, 75, 2, b"x.jpg") == 1
    assert lib.me_output_depth_map_jpeg(None, None, 4, 4, 0.0, 1.0, None, 4, 4, 75, 2, b"x.jpg") == 1
    assert lib.me_output_stereogram_jpeg(None, None, 4, 4, 0.0, 1.0, 4, 4, 0.0625, None, 75, 2, b"x.jpg") == 1
    assert lib.me_last_jpeg_encode(None, None, None) == 1


def test_resolvers(monkeypatch):
    import matrix_eyes_amd as m
    from matrix_eyes_amd.depth_pro import resolve_jpeg_encoder, resolve_jpeg_quality, resolve_jpeg_subsampling
    for name in ("MATRIX_EYES_JPEG_ENCODER", "MATRIX_EYES_JPEG_QUALITY", "MATRIX_EYES_JPEG_SUBSAMPLING"):
        monkeypatch.delenv(name, raising=False)
    assert resolve_jpeg_encoder() == "pillow" and resolve_jpeg_quality() == 75 and resolve_jpeg_subsampling() == 2
    assert resolve_jpeg_encoder("device") == "device" and resolve_jpeg_encoder("host") == "pillow"
    assert resolve_jpeg_quality(1) == 1 and resolve_jpeg_quality("100") == 100
    assert [resolve_jpeg_subsampling(v) for v in ("4:4:4", "4:2:2", "4:2:0", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    monkeypatch.setenv("MATRIX_EYES_JPEG_ENCODER", "device")
    monkeypatch.setenv("MATRIX_EYES_JPEG_QUALITY", "90")
    monkeypatch.setenv("MATRIX_EYES_JPEG_SUBSAMPLING", "4:4:4")
    assert resolve_jpeg_encoder() == "device" and resolve_jpeg_quality() == 90 and resolve_jpeg_subsampling() == 0
    for resolve, bad in ((resolve_jpeg_encoder, ("gpu", "")), (resolve_jpeg_quality, (0, 101, "high", "", "7.5")),
                         (resolve_jpeg_subsampling, ("4:1:1", 3, "", "420"))):
        for value in bad:
            with pytest.raises(m.MatrixEyesError) as e:
                resolve(value)
            assert e.value.code == 1
    from matrix_eyes_amd import cli
    for name, value in (("MATRIX_EYES_JPEG_ENCODER", "turbo"), ("MATRIX_EYES_JPEG_QUALITY", "0"), ("MATRIX_EYES_JPEG_SUBSAMPLING", "4:1:1")):
        monkeypatch.setenv(name, value)
        assert cli.main(["a.png", "b.jpg"]) == 2                       # refused up front, before anything is loaded
        monkeypatch.delenv(name)


def test_save_image_writes_jpeg(built, tmp_path):
    """the compiled host layer's save_image takes .JPG (suffix without case) through encode_jpeg with the variables' values"""
    from PIL import Image
    rgb = P.picture("shape", 37, 53)
    src = str(tmp_path / "in.png")
    Image.fromarray(rgb).save(src)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MATRIX_EYES_JPEG_")}
    for name, extra, q, s in (("a.JPG", {}, 75, 2), ("b.jpeg", {"MATRIX_EYES_JPEG_QUALITY": "95", "MATRIX_EYES_JPEG_SUBSAMPLING": "4:2:2"}, 95, 1)):
        dst = str(tmp_path / name)
        r = subprocess.run([SELFTEST, "png", src, dst], env=dict(env, **extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        with open(dst, "rb") as f:
            assert f.read() == P.reference("shape", 37, 53, q, s)[0]
    for extra, word in (({"MATRIX_EYES_JPEG_QUALITY": "101"}, "MATRIX_EYES_JPEG_QUALITY"),
                        ({"MATRIX_EYES_JPEG_QUALITY": "best"}, "MATRIX_EYES_JPEG_QUALITY"),
                        ({"MATRIX_EYES_JPEG_SUBSAMPLING": "4:1:1"}, "MATRIX_EYES_JPEG_SUBSAMPLING")):
        dst = str(tmp_path / "bad.jpg")
        r = subprocess.run([SELFTEST, "png", src, dst], env=dict(env, **extra), capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(dst), (r.returncode, r.stderr)
    r = subprocess.run([SELFTEST, "png", src, str(tmp_path / "c.tiff")], env=env, capture_output=True, text=True)
    assert r.returncode == 1 and "unsupported output image format" in r.stderr
