"""CPU tests of the PNG encoder: the yardstick (tests/png_check.py) is tested before it is used, the row-filter rule is
restated and checked on hand-made rows, the new entry points exist and reject a null context, and the encoder's
per-workgroup routines (csrc/png_chunk.h) run on the host lane by lane and write files the yardstick and Pillow read back
to the input pixels."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_check as P       # noqa: E402
import png_pictures as pic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "matrix-eyes_amd")
SELFTEST = os.path.join(PKG, "host_selftest")


def _chunk(ctype: bytes, payload: bytes) -> bytes:
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload) & 0xFFFFFFFF)


def _png(w, h, idat_payloads) -> bytes:
    """A PNG file around given IDAT payloads, every chunk with its right CRC."""
    return (P.SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            b"".join(_chunk(b"IDAT", p) for p in idat_payloads) + _chunk(b"IEND", b""))


def _rgb(h=23, w=31, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the yardstick ----------------------------------------------------------------------------------------------------

def test_reader_accepts_pillow_files():
    from PIL import Image
    for rgb in (_rgb(), pic.depth_picture(96), pic.checkerboard(9, 14), pic.flat_picture(5, 3)):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="PNG")          # Pillow writes adaptive filters: all five types occur
        px, types = P.read_png(buf.getvalue())
        assert np.array_equal(px, rgb) and types.shape == (rgb.shape[0],)
    buf = io.BytesIO()
    Image.fromarray(pic.depth_picture(200)).save(buf, format="PNG")
    assert len(set(P.read_png(buf.getvalue())[1].tolist())) >= 3


def test_reader_accepts_the_host_encoder(tmp_path):
    from PIL import Image
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
    rgb = pic.depth_picture(128)
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(rgb).save(src)
    r = subprocess.run([SELFTEST, "png", src, dst], capture_output=True, text=True)     # decode + encode_png
    assert r.returncode == 0, r.stderr
    px, types = P.read_png(open(dst, "rb").read())
    assert np.array_equal(px, rgb) and not types.any()                                   # encode_png writes filter 0


def test_reader_rejects_broken_files():
    rgb = _rgb()
    h, w, _ = rgb.shape
    stream = P.filter_stream(rgb).tobytes()
    z = zlib.compress(stream, 6)
    good = _png(w, h, [z[:100], z[100:]])
    assert np.array_equal(P.read_png(good)[0], rgb)
    # a flipped CRC byte
    bad = bytearray(good)
    bad[8 + 8 + 13 + 1] ^= 0x40                     # inside IHDR's CRC
    with pytest.raises(P.PngError, match="CRC"):
        P.read_png(bytes(bad))
    bad = bytearray(good)
    bad[-13] ^= 1                                   # the last IDAT's CRC
    with pytest.raises(P.PngError, match="CRC"):
        P.read_png(bytes(bad))
    # a truncated IDAT (its own CRC right)
    with pytest.raises(P.PngError, match="does not end|zlib"):
        P.read_png(_png(w, h, [z[:-9]]))
    # a corrupted Adler-32 behind an intact deflate stream
    with pytest.raises(P.PngError, match="zlib"):
        P.read_png(_png(w, h, [z[:-4] + bytes([z[-4] ^ 1]) + z[-3:]]))
    # bytes behind the stream, a short stream, a filter byte of 5
    with pytest.raises(P.PngError, match="behind the zlib stream"):
        P.read_png(_png(w, h, [z + b"\0"]))
    with pytest.raises(P.PngError, match="inflated to"):
        P.read_png(_png(w, h, [zlib.compress(stream[:-1])]))
    five = bytearray(stream)
    five[(3 * w + 1) * 4] = 5
    with pytest.raises(P.PngError, match="filter byte 5"):
        P.read_png(_png(w, h, [zlib.compress(bytes(five))]))
    # no BFINAL: a stream cut behind a sync flush
    c = zlib.compressobj(6)
    part = c.compress(stream) + c.flush(zlib.Z_SYNC_FLUSH)
    with pytest.raises(P.PngError, match="does not end"):
        P.read_png(_png(w, h, [part]))
    with pytest.raises(P.PngError):
        P.read_png(good[:-12])                      # no IEND
    with pytest.raises(P.PngError):
        P.read_png(good + b"x")


def test_unfilter_inverts_every_filter_type():
    rgb = _rgb(17, 13, seed=9)
    cand = P.filter_candidates(rgb)
    for types in ([0] * 17, [1] * 17, [2] * 17, [3] * 17, [4] * 17, [(i * 7) % 5 for i in range(17)]):
        t = np.array(types, np.uint8)
        stream = np.concatenate([t[:, None], cand[t, np.arange(17)]], axis=1)
        px, got = P.unfilter(stream.reshape(-1), 13, 17)
        assert np.array_equal(px, rgb) and np.array_equal(got, t)


# ---- the filter rule ----------------------------------------------------------------------------------------------------

def test_filter_rule_on_hand_made_rows():
    w = 40
    ramp = np.zeros((1, w, 3), np.uint8)
    ramp[0, :, 0] = 10 + 5 * np.arange(w)                     # a horizontal ramp: Sub leaves a constant 5
    ramp[0, :, 1] = 3 * np.arange(w)
    ramp[0, :, 2] = 200 - 2 * np.arange(w)
    assert P.choose_filters(ramp).tolist() == [1]
    row = np.random.default_rng(4).integers(0, 256, (1, w, 3), dtype=np.uint8)
    same = np.repeat(row, 4, axis=0)                           # identical rows: Up leaves zeros
    assert P.choose_filters(same)[1:].tolist() == [2, 2, 2]
    # ties go to the lowest type number: an all-zero picture costs 0 with every type; a first row without an upper
    # neighbour costs the same with None and Up, and with Sub and Paeth
    assert P.choose_filters(np.zeros((3, 5, 3), np.uint8)).tolist() == [0, 0, 0]
    first = P.filter_candidates(row)
    assert np.array_equal(first[0], first[2]) and np.array_equal(first[1], first[4])
    assert int(P.choose_filters(row)[0]) in (0, 1, 3)
    # min(v, 256 - v): 255 counts as 1, 128 as 128
    edge = np.array([[[255, 255, 255], [128, 128, 128]]], np.uint8)
    cand = P.filter_candidates(edge).astype(np.int64)
    assert np.minimum(cand, 256 - cand).sum(axis=2)[0, 0] == 3 * 1 + 3 * 128
    stream = P.filter_stream(same)
    assert stream.shape == (4, 1 + 3 * w) and not stream[1:, 1:].any()


# ---- the entry points ---------------------------------------------------------------------------------------------------

def test_entry_points_reject_a_null_context(lib):
    import ctypes as C
    ptr, n = C.c_void_p(), C.c_int64()
    assert lib.me_png_encode_rgb8(None, None, 4, 4, C.byref(ptr), C.byref(n)) == 1
    assert lib.me_output_png(None, None, 4, 4, b"x.png") == 1
    assert lib.me_output_depth_map_png(None, None, 4, 4, 0.0, 1.0, None, 4, 4, b"x.png") == 1
    assert lib.me_output_stereogram_png(None, None, 4, 4, 0.0, 1.0, 4, 4, 0.0625, None, b"x.png") == 1


def test_resolve_png_encoder(monkeypatch):
    import matrix_eyes_amd as m
    from matrix_eyes_amd.depth_pro import resolve_png_encoder
    monkeypatch.delenv("MATRIX_EYES_PNG_ENCODER", raising=False)
    assert resolve_png_encoder() == "pillow"
    assert resolve_png_encoder("device") == "device" and resolve_png_encoder("pillow") == "pillow"
    monkeypatch.setenv("MATRIX_EYES_PNG_ENCODER", "device")
    assert resolve_png_encoder() == "device"
    for bad in ("host", "gpu", ""):
        with pytest.raises(m.MatrixEyesError) as e:
            resolve_png_encoder(bad)
        assert e.value.code == 1
    monkeypatch.setenv("MATRIX_EYES_PNG_ENCODER", "zlib")
    with pytest.raises(m.MatrixEyesError):
        resolve_png_encoder()
    from matrix_eyes_amd import cli
    assert cli.main(["a.png", "b.png"]) == 2


# ---- the chunk routines, lane by lane on the host ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("png_host") / "png_chunk_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe,
                        os.path.join(ROOT, "tests", "png_chunk_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def encode(rgb, tmp_path):
        h, w, _ = rgb.shape
        rgb.tofile(str(tmp_path / "in.rgb"))
        r = subprocess.run([exe, str(tmp_path / "in.rgb"), str(w), str(h), str(tmp_path / "out.png")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return open(tmp_path / "out.png", "rb").read()
    return encode


def _check_file(data, rgb):
    from PIL import Image
    px, types = P.read_png(data)
    assert np.array_equal(px, rgb)
    assert np.array_equal(types, P.choose_filters(rgb))
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), rgb)


def test_host_run_small_shapes_and_noise(host_encoder, tmp_path):
    for h, w in [(1, 1), (1, 7), (7, 1), (61, 97), (129, 257)]:
        rgb = pic.noise_picture(h, w, seed=h * 1000 + w)
        data = host_encoder(rgb, tmp_path)
        _check_file(data, rgb)
        assert len(data) <= 1.001 * h * (3 * w + 1) + 1024       # never worse than stored


def test_host_run_chunk_boundaries(host_encoder, tmp_path):
    shapes = pic.around_chunks()
    assert sorted(shapes) == [-1, 0, 1]
    for delta, (h, w) in shapes.items():
        assert (h * (3 * w + 1) - delta) % 65536 == 0
        for rgb in (pic.noise_picture(h, w), pic.stereogram_like(h, w, pattern=120)):
            _check_file(host_encoder(rgb, tmp_path), rgb)


def test_host_run_structure(host_encoder, tmp_path):
    # matches of length 258 end to end, across chunk boundaries, and a boundary inside a match and inside a row
    flat = pic.flat_picture(70, 1000)
    data = host_encoder(flat, tmp_path)
    _check_file(data, flat)
    assert len(data) < 4000
    cb = pic.checkerboard(90, 777)
    data = host_encoder(cb, tmp_path)
    _check_file(data, cb)
    assert len(data) < 0.05 * cb.size
    alt = pic.alternating_rows()
    _check_file(host_encoder(alt, tmp_path), alt)                # repeats at 80 KB only: nothing may reach that far
    st = pic.stereogram_like(120, 1600, pattern=200)
    data = host_encoder(st, tmp_path)
    _check_file(data, st)
    assert len(data) < 0.5 * st.size                             # the 600-byte repeat is found
    dp = pic.depth_picture(300)
    data = host_encoder(dp, tmp_path)
    _check_file(data, dp)
    assert len(data) < 2 * len(zlib.compress(np.concatenate([np.zeros((300, 1), np.uint8),
                                                              dp.reshape(300, -1)], axis=1).tobytes(), 6))


def test_host_run_is_deterministic(host_encoder, tmp_path):
    rgb = pic.depth_picture(200)
    assert host_encoder(rgb, tmp_path) == host_encoder(rgb, tmp_path)
