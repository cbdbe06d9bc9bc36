"""CPU tests of the GPU PNG decoder's arithmetic and interface: csrc/png_recon.h -- the routines the kernels of
csrc/png_decode.hip are made of -- compiled as plain C++ (tests/png_recon_host.cpp) and run in the kernels' order over the
host decoder's parse_png_header / inflate_png must write exactly the bytes of `host_selftest decode <in> <out.ppm> oriented`,
on the file list of tests/png_files.py, for all eight orientations, and under the address and undefined-behaviour
sanitizers also on refused and corrupted files.  me_png_info needs no GPU; the device entry points reject a null
context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_files as P  # noqa: E402

ROOT = P.ROOT
SOURCES = [os.path.join(ROOT, "tests", "png_recon_host.cpp"), os.path.join(P.PKG, "host", "png_decoder.cpp")]


def test_the_shared_header_is_there():
    text = open(os.path.join(P.PKG, "csrc", "png_recon.h")).read()
    assert "hipLaunch" not in text and "hip_runtime" not in text          # plain routines: the host decoder includes it
    for name in ("paeth", "recon", "adam7_pass", "pixel_rgb", "dest_index"):
        assert name + "(" in text, name


def _build(exe, *extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-o", exe, *SOURCES, "-lz"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()                      # host_selftest, the yardstick
    assert os.path.exists(P.SELFTEST)


@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("png_host") / "png_recon_host"))


@pytest.fixture(scope="module")
def driver_san(built, tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("png_host_san") / "png_recon_host_san"),
                  "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _run(exe, data, tmp_path, orientation=1, name="f", band_rows=None):
    src, dst = str(tmp_path / (name + ".png")), str(tmp_path / (name + ".recon.ppm"))
    with open(src, "wb") as f:
        f.write(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst, str(orientation)] + ([str(band_rows)] if band_rows else []), capture_output=True, text=True,
                       env=env)
    return r, (P.read_ppm(dst) if r.returncode == 0 else None)


def _words(err, tag):
    """the message behind the file's name"""
    return err.strip().split(tag + ": ", 1)[1]


def _same_as_host(exe, data, tmp_path, name, orientation, band_rows=None):
    rc, want, err = P.host_decode(data, tmp_path, oriented=True, name=name)
    assert rc == 0, (name, err)
    r, got = _run(exe, data, tmp_path, orientation, name, band_rows)
    assert r.returncode == 0, (name, r.stdout + r.stderr)
    assert got.shape == want.shape, name
    bad = int((got != want).sum())
    assert bad == 0, f"{name} orientation {orientation}: {bad} of {want.size} bytes differ"
    return want


def test_the_generator_and_the_host_decoder_agree(built, tmp_path):
    """the files are what they claim: the host decoder's pixels are into_rgb8 of the samples the generator packed"""
    for ctype, depth in P.TABLE:
        for il in (0, 1):
            px = P.samples(33, 17, ctype, depth, seed=ctype * 16 + depth)
            plte = P.palette(1 << depth) if ctype == 3 else None
            rc, got, err = P.host_decode(P.make(33, 17, ctype, depth, il, px=px, plte=plte), tmp_path, name=f"t{ctype}{depth}{il}")
            assert rc == 0, err
            assert np.array_equal(got, P.expected_rgb(px, ctype, depth, plte)), (ctype, depth, il)
    edge = np.array(P.EDGE16, np.uint16).reshape(1, 8, 1)
    rc, got, _ = P.host_decode(P.make(8, 1, 0, 16, px=edge), tmp_path, name="edge")
    assert rc == 0 and got[0, :, 0].tolist() == [0, 0, 0, 127, 128, 255, 255, 255]       # (v + 128) / 257


@pytest.mark.parametrize("orientation", range(1, 9))
def test_driver_equals_the_host_decoder(driver, tmp_path, orientation):
    """every generated file; the orientation is the file's own eXIf value, which the host applies"""
    for name, make in P.FILES:
        _same_as_host(driver, P.with_exif(make(), orientation), tmp_path, name, orientation)


def test_driver_equals_the_host_decoder_under_sanitizers(driver_san, tmp_path):
    for k, (name, make) in enumerate(P.FILES):
        o = 1 + k % 8
        _same_as_host(driver_san, P.with_exif(make(), o), tmp_path, name, o)


@pytest.mark.parametrize("band_rows", (1, 2, 63, 64, 65, 300))
def test_bands_do_not_change_the_bytes(driver, tmp_path, band_rows):
    for name in ("rows65", "rows257", "rows-i", "tiles", "rgba16-cycle-i", "s5x70i1"):
        _same_as_host(driver, dict(P.FILES)[name](), tmp_path, name, 1, band_rows)


def test_orientation_and_metadata(built, tmp_path):
    for o in range(1, 9):
        data = dict(P.FILES)[f"exif{o}"]()
        _, plain, _ = P.host_decode(data, tmp_path, oriented=False, name=f"p{o}")
        _, turned, _ = P.host_decode(data, tmp_path, oriented=True, name=f"o{o}")
        assert np.array_equal(P.orient(plain, o), turned)                  # the restated remap is the host's
        src = str(tmp_path / f"m{o}.png")
        with open(src, "wb") as f:
            f.write(data)
        r = subprocess.run([P.SELFTEST, "decode", src, str(tmp_path / "m.ppm")], capture_output=True, text=True)
        assert r.stdout.split()[:2] == [str(o), "35"], r.stdout
    _, twice, _ = P.host_decode(dict(P.FILES)["exif-twice"](), tmp_path, oriented=True, name="twice")
    assert twice.shape == (13, 5, 3)                                       # the last eXIf chunk (6) wins over the first (3)


def test_refusals_carry_the_host_message(driver_san, tmp_path):
    """parse_png_header and inflate_png refuse in decode_png's words, and a defect the kernels' path meets (filter byte,
    palette index) is answered by the host decoder's first defect in stream order"""
    for name, make, words in P.REFUSED:
        data = make()
        rc, _, err = P.host_decode(data, tmp_path, name=name)
        assert rc != 0 and words in err, (name, err)
        r, _ = _run(driver_san, data, tmp_path, 1, name)
        assert r.returncode == 3, (name, r.returncode, r.stderr[-2000:])
        assert _words(err, ".png") == _words(r.stderr, "<png>"), name


def test_corrupted_files_under_sanitizers(driver_san, tmp_path):
    """Byte-flipped and truncated copies of good files: the driver decodes to the host decoder's bytes or refuses with its
    words -- never a sanitizer report.  (The fuzzing lives here, not on the GPU.)"""
    rng = np.random.default_rng(77)
    files = dict(P.FILES)
    k = 0
    for base_name in ("t3d4i1", "t2d8i0", "t6d16i1", "t0d1i0", "idat-split", "exif6"):
        base = files[base_name]()
        for _ in range(10):
            data = bytearray(base)
            kind = int(rng.integers(0, 3))
            if kind == 0:
                for _ in range(int(rng.integers(1, 4))):
                    data[int(rng.integers(8, len(data)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:
                data = data[:int(rng.integers(8, len(data)))]
            else:                                                         # inside the header and the first chunks
                data[int(rng.integers(8, 60))] = int(rng.integers(0, 256))
            k += 1
            name = f"fuzz{k}"
            rc, want, err = P.host_decode(bytes(data), tmp_path, name=name)
            r, got = _run(driver_san, bytes(data), tmp_path, 1, name)
            assert r.returncode in (0, 3), (name, r.returncode, r.stderr[-2000:])
            assert (rc == 0) == (r.returncode == 0), (name, rc, r.returncode, err, r.stderr)
            if rc == 0:
                assert np.array_equal(got, want), name
            else:
                assert _words(err, ".png") == _words(r.stderr, "<png>"), name


def _buf(data):
    return (C.c_uint8 * len(data)).from_buffer_copy(data)


def test_png_info_needs_no_gpu(lib):
    data = dict(P.FILES)["exif6"]()
    w, h, off, n = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    assert lib.me_png_info(_buf(data), len(data), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 0
    assert (w.value, h.value) == (13, 5)                          # as coded: the orientation is the caller's business
    at = data.index(b"eXIf") + 4
    assert off.value == at and data[at:at + 2] == b"II" and n.value == len(P.exif_block(6, 35))
    twice = dict(P.FILES)["exif-twice"]()
    assert lib.me_png_info(_buf(twice), len(twice), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 0
    assert off.value == twice.rindex(b"eXIf") + 4                 # the last one
    plain = P.make(33, 17, 0, 2, 1)
    assert lib.me_png_info(_buf(plain), len(plain), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 0
    assert (w.value, h.value, off.value, n.value) == (33, 17, 0, 0)
    refused = {name: (make, words) for name, make, words in P.REFUSED}
    for name in ("pair-2-4", "interlace2", "cut-chunk", "ctype5", "depth3"):
        bad = refused[name][0]()
        assert lib.me_png_info(_buf(bad), len(bad), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 1, name
        assert refused[name][1].encode() in lib.me_last_error(None), name
    short = refused["short-stream"][0]()                          # the header is fine: the stream is not looked at
    assert lib.me_png_info(_buf(short), len(short), C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 0
    assert lib.me_png_info(None, 0, C.byref(w), C.byref(h), C.byref(off), C.byref(n)) == 1
    assert lib.me_png_info(_buf(plain), len(plain), None, C.byref(h), C.byref(off), C.byref(n)) == 1


def test_host_decoder_through_the_library(lib, built, tmp_path):
    """me_op_png_decode_host (the in-process baseline of tools/bench_png_decode.py) is the host decoder"""
    data = dict(P.FILES)["t6d16i1"]()
    _, want, _ = P.host_decode(data, tmp_path, oriented=False)
    out = np.zeros((17, 33, 3), np.uint8)
    assert lib.me_op_png_decode_host(_buf(data), len(data), C.c_void_p(out.ctypes.data), 33, 17) == 0
    assert np.array_equal(out, want)
    assert lib.me_op_png_decode_host(_buf(data), len(data), C.c_void_p(out.ctypes.data), 17, 33) == -2
    assert lib.me_op_png_decode_host(None, 0, C.c_void_p(out.ctypes.data), 33, 17) == -1
    for name, make, words in P.REFUSED:
        bad = make()
        assert lib.me_op_png_decode_host(_buf(bad), len(bad), C.c_void_p(out.ctypes.data), 33, 17) == -3, name
        assert words.encode() in lib.me_last_error(None), name


def test_null_context_is_rejected(lib):
    data = P.make(8, 8)
    out = np.zeros((8, 8, 3), np.uint8)
    dst = C.c_void_p(out.ctypes.data)
    assert lib.me_png_decode_rgb8(None, _buf(data), len(data), 1, dst, 8, 8) == 1
    assert lib.me_png_decode_resized_rgb8(None, _buf(data), len(data), 1, dst, 8, 8) == 1
    assert lib.me_last_png_timing(None, None) == 1
    assert lib.me_op_png_unfilter(None, dst, 8 * 25, 8, 8, 8, 2, 0, 0, dst) == 1


def test_switch_values(monkeypatch):
    import matrix_eyes_amd as m
    monkeypatch.delenv("MATRIX_EYES_PNG_DECODER", raising=False)
    assert m.depth_pro.resolve_png_decoder(None) == "pillow"
    assert m.depth_pro.resolve_png_decoder("pillow") == "pillow"
    assert m.depth_pro.resolve_png_decoder("host") == "pillow"
    assert m.depth_pro.resolve_png_decoder("device") == "device"
    monkeypatch.setenv("MATRIX_EYES_PNG_DECODER", "device")
    assert m.depth_pro.resolve_png_decoder(None) == "device"
    with pytest.raises(m.MatrixEyesError):
        m.depth_pro.resolve_png_decoder("gpu")
