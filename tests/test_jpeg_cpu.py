"""CPU tests of the GPU JPEG decoder's arithmetic and interface: csrc/jpeg_recon.h -- the routines the kernels of
csrc/jpeg_decode.hip are made of -- compiled as plain C++ (tests/jpeg_recon_host.cpp, -ffp-contract=off) and run over the host
decoder's coefficient interface must write exactly the bytes of `host_selftest decode <in> <out.ppm> oriented`, on the file
list of tests/jpeg_files.py, for all eight orientations, and under the address and undefined-behaviour sanitizers also on
corrupted files.  me_jpeg_info needs no GPU; the device entry points reject a null context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_files as J  # noqa: E402

ROOT = J.ROOT
SOURCES = [os.path.join(ROOT, "tests", "jpeg_recon_host.cpp"),
           os.path.join(J.PKG, "host", "jpeg_decoder.cpp"),
           os.path.join(J.PKG, "csrc", "jpeg_basis.cpp")]


def _build(exe, *extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", *extra, "-o", exe, *SOURCES],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()                      # host_selftest, the yardstick
    assert os.path.exists(J.SELFTEST)


@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_recon_host"))


@pytest.fixture(scope="module")
def driver_san(built, tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("jpeg_host_san") / "jpeg_recon_host_san"),
                  "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _run(exe, data, tmp_path, orientation=1, name="f"):
    src, dst = str(tmp_path / (name + ".jpg")), str(tmp_path / (name + ".recon.ppm"))
    with open(src, "wb") as f:
        f.write(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst, str(orientation)], capture_output=True, text=True, env=env)
    return r, (J.read_ppm(dst) if r.returncode == 0 else None)


def _same_as_host(exe, data, tmp_path, name):
    rc, want, err = J.host_decode(data, tmp_path, oriented=True, name=name)
    assert rc == 0, err
    r, got = _run(exe, data, tmp_path, 1, name)
    assert r.returncode == 0, r.stdout + r.stderr
    assert got.shape == want.shape, name
    bad = int((got != want).sum())
    assert bad == 0, f"{name}: {bad} of {want.size} bytes differ"


def test_driver_equals_the_host_decoder(driver, tmp_path):
    for name, make in J.FILES:
        _same_as_host(driver, make(), tmp_path, name)


def test_driver_equals_the_host_decoder_under_sanitizers(driver_san, tmp_path):
    for name, make in J.FILES:
        _same_as_host(driver_san, make(), tmp_path, name)


def test_observable_branches(driver, tmp_path):
    """the RGB pass-through and the DC-only shortcut change bytes, so the equality above covers them"""
    data = J.rgb_passthrough()
    _, rgb, _ = J.host_decode(data, tmp_path, name="rgb")
    _, ycc, _ = J.host_decode(J.plain(50, 30, subsampling=0, quality=92, seed=13), tmp_path, name="ycc")
    assert (rgb != ycc).mean() > 0.9
    for name in ("restart-rows", "restart-blocks"):
        assert b"\xff\xdd" in dict(J.FILES)[name]()


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientations(driver, tmp_path, orientation):
    data = J.with_exif(orientation)
    rc, want, err = J.host_decode(data, tmp_path, oriented=True, name=f"o{orientation}")      # the file's own EXIF value
    assert rc == 0, err
    r, got = _run(driver, data, tmp_path, orientation, f"o{orientation}")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(got, want)
    _, plain, _ = J.host_decode(data, tmp_path, oriented=False, name=f"p{orientation}")
    assert np.array_equal(J.orient(plain, orientation), want)                                  # the restated remap is the host's


def test_refusals_carry_the_host_message(driver, tmp_path):
    for name, data, words in (("cmyk", J.cmyk(), "4 components"), ("trunc", J.plain(123, 77)[:300], None)):
        rc, want, err = J.host_decode(data, tmp_path, name=name)
        r, got = _run(driver, data, tmp_path, 1, name)
        if rc == 0:
            assert r.returncode == 0 and np.array_equal(got, want)
            continue
        assert r.returncode == 3, (name, r.returncode, r.stderr)
        # the same words behind the file's name
        assert err.strip().split(".jpg: ", 1)[1] == r.stderr.strip().split("<jpeg>: ", 1)[1]
        if words:
            assert words in r.stderr
    # an undefined quantisation table and a fractional sampling ratio: refused by the reconstruction, with its words
    base = bytearray(J.plain(64, 48, subsampling=2, quality=90))
    sof = J._sof(base)
    bad_tq = bytearray(base)
    bad_tq[sof + 1 + 2] = 3                                       # luma names table 3, which no DQT defines
    frac = bytearray(J.plain(64, 48, subsampling=0, quality=90))
    frac = frac[:J._sos(frac) - 4] + b"\xff\xd9"                  # tables and frame header, no scan: all coefficients zero
    s = J._sof(frac)
    frac[s + 1 + 1] = 0x33                                        # luma 3x3 ...
    frac[s + 1 + 3 + 1] = 0x22                                    # ... over chroma 2x2
    for name, data, words in (("badtq", bytes(bad_tq), "undefined quantisation table"), ("frac", bytes(frac), "fractional")):
        rc, _, err = J.host_decode(data, tmp_path, name=name)
        r, _ = _run(driver, data, tmp_path, 1, name)
        assert rc != 0, name
        assert r.returncode == 3 and err.strip().split(".jpg: ", 1)[1] == r.stderr.strip().split("<jpeg>: ", 1)[1], (name, err, r.stderr)
        assert words in err, (name, err)


def test_corrupted_files_under_sanitizers(driver_san, tmp_path):
    """Random corruptions and truncations: the driver decodes to the host decoder's bytes or refuses with its words --
    never a sanitizer report.  (The fuzzing lives here, not on the GPU.)"""
    rng = np.random.default_rng(77)
    seeds = [J.plain(64, 48, 2, False, 85), J.plain(37, 29, 1, True, 85), J.restart_rows(), J.grey()]
    k = 0
    for base in seeds:
        for _ in range(12):
            data = bytearray(base)
            kind = int(rng.integers(0, 3))
            if kind == 0:
                for _ in range(int(rng.integers(1, 6))):
                    data[int(rng.integers(2, len(data)))] = int(rng.integers(0, 256))
            elif kind == 1:
                data = data[:int(rng.integers(4, len(data)))]
            else:
                at = int(rng.integers(2, len(data)))
                data[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8))
            k += 1
            name = f"fuzz{k}"
            rc, want, err = J.host_decode(bytes(data), tmp_path, name=name)
            r, got = _run(driver_san, bytes(data), tmp_path, 1, name)
            assert r.returncode in (0, 3), (name, r.returncode, r.stderr[-2000:])
            assert (rc == 0) == (r.returncode == 0), (name, rc, r.returncode, err, r.stderr)
            if rc == 0:
                assert np.array_equal(got, want), name
            else:
                assert err.strip().split(".jpg: ", 1)[1] == r.stderr.strip().split("<jpeg>: ", 1)[1], name


def test_jpeg_info_needs_no_gpu(lib):
    data = J.with_exif(6)
    w, h, off, n = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert lib.me_jpeg_info(buf, len(data), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 0
    assert (w.value, h.value) == (123, 77)                       # as coded: the orientation is the caller's business
    at = data.index(b"Exif\x00\x00") + 6
    assert off.value == at and n.value > 8
    assert data[at:at + 2] in (b"II", b"MM")                     # the TIFF header
    seg = data.index(b"\xff\xe1")
    assert off.value + n.value == seg + 2 + ((data[seg + 2] << 8) | data[seg + 3])     # to the end of the APP1 segment
    plain = J.plain(64, 48)
    buf = (C.c_uint8 * len(plain)).from_buffer_copy(plain)
    assert lib.me_jpeg_info(buf, len(plain), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 0
    assert (w.value, h.value, off.value, n.value) == (64, 48, 0, 0)
    cmyk = J.cmyk()
    buf = (C.c_uint8 * len(cmyk)).from_buffer_copy(cmyk)
    assert lib.me_jpeg_info(buf, len(cmyk), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 1
    assert b"4 components" in lib.me_last_error(None)
    assert lib.me_jpeg_info(None, 0, C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 1
    assert lib.me_jpeg_info(buf, len(cmyk), None, C.byref(h), C.byref(off), C.byref(n)) == 1


def test_host_decoder_through_the_library(lib, built, tmp_path):
    """me_op_jpeg_decode_host (the in-process baseline of tools/bench_jpeg.py) is the host decoder"""
    data = J.plain(123, 77)
    _, want, _ = J.host_decode(data, tmp_path, oriented=False)
    out = np.zeros((77, 123, 3), np.uint8)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert lib.me_op_jpeg_decode_host(buf, len(data), C.c_void_p(out.ctypes.data), 123, 77) == 0
    assert np.array_equal(out, want)
    assert lib.me_op_jpeg_decode_host(buf, len(data), C.c_void_p(out.ctypes.data), 77, 123) < 0
    assert lib.me_op_jpeg_decode_host(None, 0, C.c_void_p(out.ctypes.data), 123, 77) < 0


def test_null_context_is_rejected(lib):
    data = J.plain(8, 8)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    out = np.zeros((8, 8, 3), np.uint8)
    dst = C.c_void_p(out.ctypes.data)
    assert lib.me_jpeg_decode_rgb8(None, buf, len(data), 1, dst, 8, 8) == 1
    assert lib.me_jpeg_decode_resized_rgb8(None, buf, len(data), 1, dst, 8, 8) == 1
    assert lib.me_last_jpeg_timing(None, None) == 1


def test_switch_values():
    import matrix_eyes_amd as m
    assert m.depth_pro.resolve_jpeg_decoder(None) in ("pillow", "device")
    assert m.depth_pro.resolve_jpeg_decoder("device") == "device"
    with pytest.raises(m.MatrixEyesError):
        m.depth_pro.resolve_jpeg_decoder("gpu")
