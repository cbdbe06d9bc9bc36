"""JPEG files shared by tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py, and the yardstick both compare against: the
host decoder (host/jpeg_decoder.cpp) behind `host_selftest decode <in> <out.ppm> [oriented]`.

Every generator returns the bytes of one file; FILES lists (name, maker) pairs.  Pillow writes the plain files; the
sampling layouts Pillow does not write (4:4:0, 4:1:1) and the RGB pass-through are made by patching header bytes of a
file whose MCUs hold the same blocks, so the scans still decode (to a scrambled picture, which an equality test does
not mind)."""
import io
import os
import subprocess

import numpy as np

from orient_ref import orient  # noqa: F401  (J.orient: apply_orientation restated)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "matrix-eyes_amd")
SELFTEST = os.path.join(PKG, "host_selftest")

SIZES = [(123, 77), (64, 48), (1, 19), (3, 2), (2, 2), (4, 3), (5, 1)]


def photo(w, h, seed):
    """tests/test_gpu_resample.py's photo(): smooth, noisy, colourful, with blocks of pure black / white"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([127 + 100 * np.sin(x / 17.0 + y / 29.0), 127 + 100 * np.cos(x / 11.0 - y / 23.0),
                  127 + 90 * np.sin((x + y) / 31.0)], -1) + rng.normal(0, 6, (h, w, 3)).astype(np.float32)
    img = np.clip(a, 0, 255).astype(np.uint8)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y0:y0 + int(rng.integers(1, max(2, h // 6))), x0:x0 + int(rng.integers(1, max(2, w // 6)))] = 255 * int(rng.integers(0, 2))
    return img


def save(img, **kw) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    (img if isinstance(img, Image.Image) else Image.fromarray(img)).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def plain(w, h, subsampling=2, progressive=False, quality=90, seed=3, **kw) -> bytes:
    return save(photo(w, h, seed), quality=quality, subsampling=subsampling, progressive=progressive, **kw)


def _sof(data: bytes) -> int:
    """offset of the SOF0 / SOF2 marker's component count byte"""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, pos
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if marker in (0xC0, 0xC1, 0xC2):
            return pos + 4 + 5
        pos += 2 + length
    raise AssertionError("no SOF")


def _sos(data: bytes) -> int:
    """offset of the first SOS marker's component count byte"""
    pos = 2
    while pos + 4 <= len(data):
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if marker == 0xDA:
            return pos + 4
        pos += 2 + length
    raise AssertionError("no SOS")


def patch_luma_sampling(data: bytes, old: int, new: int) -> bytes:
    at = _sof(data) + 1 + 1                 # count, then (id, sampling, tq) of component 0
    assert data[at] == old, hex(data[at])
    out = bytearray(data)
    out[at] = new
    return bytes(out)


def s440() -> bytes:
    """4:4:0 (luma 1x2: the 1x2 filter on chroma) from a 64 x 64 4:2:2 file"""
    return patch_luma_sampling(plain(64, 64, subsampling=1, quality=92, seed=11), 0x21, 0x12)


def s411() -> bytes:
    """4:1:1 (luma 4x1: replication with ratio 4) from a 96 x 64 4:2:0 file"""
    return patch_luma_sampling(plain(96, 64, subsampling=2, quality=92, seed=12), 0x22, 0x41)


def rgb_passthrough() -> bytes:
    """component ids 'R', 'G', 'B' in SOF and SOS of a 50 x 30 4:4:4 file, and no JFIF-independent Adobe marker"""
    data = bytearray(plain(50, 30, subsampling=0, quality=92, seed=13))
    sof, sos = _sof(data), _sos(data)
    assert data[sof] == 3 and data[sos] == 3
    for k, ident in enumerate(b"RGB"):
        assert data[sof + 1 + 3 * k] == k + 1 and data[sos + 1 + 2 * k] == k + 1
        data[sof + 1 + 3 * k] = ident
        data[sos + 1 + 2 * k] = ident
    return bytes(data)


def grey() -> bytes:
    from PIL import Image
    return save(Image.fromarray(photo(100, 60, 14)).convert("L"), quality=90)


def restart_rows() -> bytes:
    data = plain(203, 111, subsampling=2, quality=90, seed=15, restart_marker_rows=2)
    assert b"\xff\xdd" in data
    return data


def restart_blocks() -> bytes:
    data = plain(203, 111, subsampling=1, quality=90, seed=16, restart_marker_blocks=5)
    assert b"\xff\xdd" in data
    return data


def cmyk() -> bytes:
    from PIL import Image
    return save(Image.fromarray(photo(32, 32, 6)).convert("CMYK"))


def with_exif(orientation: int, w=123, h=77) -> bytes:
    """tests/test_host_cpp.py::test_cli_jpeg_photo_with_exif's way: the orientation in IFD0, a focal length in the Exif IFD"""
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = orientation
    exif.get_ifd(0x8769)[0xA405] = 28
    return save(photo(w, h, 3), quality=90, subsampling=2, exif=exif)


def grid_files():
    """sizes x subsampling x scan type x quality"""
    out = []
    for (w, h) in SIZES:
        for sub in (0, 1, 2):
            for prog in (False, True):
                for q in (95, 55):
                    name = f"{w}x{h}-s{sub}-{'prog' if prog else 'base'}-q{q}"
                    out.append((name, lambda w=w, h=h, sub=sub, prog=prog, q=q: plain(w, h, sub, prog, q, seed=3)))
    return out


SPECIAL = [
    ("517x333-s2", lambda: plain(517, 333, 2, False, 90, seed=21)),
    ("grey", grey),
    ("restart-rows", restart_rows),
    ("restart-blocks", restart_blocks),
    ("s440", s440),
    ("s411", s411),
    ("rgb", rgb_passthrough),
]
FILES = grid_files() + SPECIAL


def read_ppm(path) -> np.ndarray:
    data = open(path, "rb").read()
    assert data[:3] == b"P6\n"
    head, rest = data[3:].split(b"\n255\n", 1)
    w, h = (int(v) for v in head.split())
    assert len(rest) == w * h * 3, (w, h, len(rest))
    return np.frombuffer(rest, np.uint8).reshape(h, w, 3)


def host_decode(data: bytes, tmp_dir, oriented=True, name="f"):
    """(returncode, pixels or None, stderr) of the host decoder followed by apply_orientation with the file's own EXIF
    value"""
    src, dst = os.path.join(str(tmp_dir), name + ".jpg"), os.path.join(str(tmp_dir), name + ".ppm")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([SELFTEST, "decode", src, dst] + (["oriented"] if oriented else []), capture_output=True, text=True)
    if r.returncode != 0:
        return r.returncode, None, r.stderr
    return 0, read_ppm(dst), r.stderr
