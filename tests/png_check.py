"""An independent reader for 8-bit RGB PNG files, written against the PNG and zlib specifications with numpy and the
standard library: the yardstick of the PNG encoder tests.  `read_png` checks everything it reads and raises PngError;
`choose_filters` / `filter_stream` restate the encoder's row-filter rule."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


class PngError(ValueError):
    pass


def chunks(data: bytes):
    """[(type, payload)] with every length and CRC checked."""
    if data[:8] != SIGNATURE:
        raise PngError("bad signature")
    pos, out = 8, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk header")
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        ctype = data[pos + 4:pos + 8]
        end = pos + 8 + length
        if end + 4 > len(data):
            raise PngError(f"chunk {ctype!r} runs past the end of the file")
        payload = data[pos + 8:end]
        (crc,) = struct.unpack(">I", data[end:end + 4])
        if crc != (zlib.crc32(ctype + payload) & 0xFFFFFFFF):
            raise PngError(f"chunk {ctype!r} at {pos}: CRC mismatch")
        out.append((ctype, payload))
        pos = end + 4
        if ctype == b"IEND":
            break
    if not out or out[-1][0] != b"IEND" or out[-1][1] != b"":
        raise PngError("no IEND")
    if pos != len(data):
        raise PngError("bytes behind IEND")
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(stream: np.ndarray, w: int, h: int):
    """[h, 1 + 3w] filtered rows -> ([h, w, 3] pixels, [h] filter bytes)"""
    rows = stream.reshape(h, 1 + 3 * w)
    types = rows[:, 0].copy()
    if types.max(initial=0) > 4:
        raise PngError(f"filter byte {int(types.max())}")
    f = rows[:, 1:].reshape(h, w, 3).astype(np.int32)
    # A pixel needs its left, upper and upper-left neighbours reconstructed: the pixels of one anti-diagonal are
    # independent of each other, so the picture is rebuilt diagonal by diagonal.  rec has a zero row and column in front.
    rec = np.zeros((h + 1, w + 1, 3), np.int32)
    for d in range(h + w - 1):
        ys = np.arange(max(0, d - w + 1), min(h - 1, d) + 1)
        xs = d - ys
        a, b, c = rec[ys + 1, xs], rec[ys, xs + 1], rec[ys, xs]
        ft = types[ys][:, None]
        pred = np.where(ft == 0, 0, np.where(ft == 1, a, np.where(ft == 2, b, np.where(ft == 3, (a + b) >> 1,
                                                                                      _paeth(a, b, c)))))
        rec[ys + 1, xs + 1] = (f[ys, xs] + pred) & 255
    return rec[1:, 1:].astype(np.uint8), types


def read_png(data: bytes):
    """-> (pixels [h, w, 3] uint8, filter bytes [h] uint8).  Colour type 2, bit depth 8, no interlace only."""
    cs = chunks(data)
    if cs[0][0] != b"IHDR" or len(cs[0][1]) != 13:
        raise PngError("IHDR is not the first chunk")
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    if (depth, ctype, comp, filt, interlace) != (8, 2, 0, 0, 0) or w == 0 or h == 0:
        raise PngError(f"IHDR {w}x{h} depth {depth} colour type {ctype} {comp}/{filt}/{interlace}")
    idat = [i for i, (t, _) in enumerate(cs) if t == b"IDAT"]
    if not idat or idat != list(range(idat[0], idat[0] + len(idat))):
        raise PngError("IDAT chunks missing or not consecutive")
    d = zlib.decompressobj()
    try:
        raw = d.decompress(b"".join(p for t, p in cs if t == b"IDAT"))
        raw += d.flush()
    except zlib.error as e:
        raise PngError(f"zlib: {e}") from e
    if not d.eof:
        raise PngError("the zlib stream does not end (BFINAL / Adler-32 missing)")
    if d.unused_data:
        raise PngError(f"{len(d.unused_data)} bytes behind the zlib stream")
    if len(raw) != h * (3 * w + 1):
        raise PngError(f"inflated to {len(raw)} bytes, expected {h * (3 * w + 1)}")
    return unfilter(np.frombuffer(raw, np.uint8), w, h)


# ---- the encoder's row-filter rule, restated ---------------------------------------------------------------------------

def filter_candidates(rgb: np.ndarray):
    """[5, h, 3w] uint8: every row filtered with every type (bpp = 3, the row above the first is zeros)."""
    h, w, _ = rgb.shape
    x = rgb.reshape(h, 3 * w).astype(np.int16)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    out = np.empty((5, h, 3 * w), np.uint8)
    out[0] = x
    out[1] = (x - a) & 255
    out[2] = (x - b) & 255
    out[3] = (x - ((a + b) >> 1)) & 255
    out[4] = (x - _paeth(a, b, c)) & 255
    return out


def choose_filters(rgb: np.ndarray):
    """Per row the type with the smallest sum of min(v, 256 - v) over the filtered bytes, ties to the lowest number."""
    cand = filter_candidates(rgb)
    # min(v, 256 - v) in uint8 arithmetic: 256 - v wraps to -v, and both sides are 0 for v = 0
    cost = np.minimum(cand, np.negative(cand)).sum(axis=2, dtype=np.int64)   # [5, h]
    return np.argmin(cost, axis=0).astype(np.uint8)                          # argmin returns the first minimum


def filter_stream(rgb: np.ndarray):
    """The filtered stream [h, 1 + 3w] the encoder compresses."""
    cand = filter_candidates(rgb)
    cost = np.minimum(cand, np.negative(cand)).sum(axis=2, dtype=np.int64)
    types = np.argmin(cost, axis=0).astype(np.uint8)
    h = rgb.shape[0]
    return np.concatenate([types[:, None], cand[types, np.arange(h)]], axis=1)
