"""PNG files shared by tests/test_png_decode_cpu.py and tests/test_gpu_png_decode.py, and the yardstick both compare against:
the host decoder (host/png_decoder.cpp) behind `host_selftest decode <in> <out.ppm> [oriented]`.

The files are made by hand, with zlib and numpy: Pillow writes neither interlaced files nor chosen row filters.  make()
takes the samples, splits them into the Adam7 passes, packs the rows (big-endian bit order below 8 bits, big-endian
16-bit samples), applies the filter the schedule names for every row of every pass and deflates the stream into one or
more IDAT chunks.  FILES lists (name, maker) pairs of accepted files, REFUSED (name, maker, words) of files the decoder
refuses with `words`; expected_rgb() restates into_rgb8 in numpy."""
import os
import struct
import subprocess
import zlib

import numpy as np

from orient_ref import orient  # noqa: F401  (P.orient: apply_orientation restated)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "matrix-eyes_amd")
SELFTEST = os.path.join(PKG, "host_selftest")

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# PNG specification, table 11.1
TABLE = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
CYCLE = (4, 3, 2, 1, 0, 4, 4, 3)
EDGE16 = (0, 127, 128, 32767, 32768, 65407, 65408, 65535)
GROUP_ROWS, BAND_ROWS, TILE_BYTES = 64, 256, 216     # of csrc/png_decode.hip: a wave's rows, the default band, the LDS tile


def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def samples(w, h, ctype, depth, seed=1):
    """[h, w, channels] uint16 below 2^depth: smooth ramps plus noise, so that every filter has something to predict"""
    rng = np.random.default_rng(seed)
    ch = CHANNELS[ctype]
    y, x = np.mgrid[0:h, 0:w]
    top = (1 << depth) - 1
    base = np.stack([(x * (3 + c) + y * (5 - c)) for c in range(ch)], -1) * max(1, top // 61)
    noise = rng.integers(0, max(2, top // 5 + 1), (h, w, ch))
    return ((base + noise) % (top + 1)).astype(np.uint16)


def pack_rows(px, depth):
    """[rows, w, channels] samples -> [rows, stride] bytes"""
    rows, w, ch = px.shape
    if depth == 8:
        return px.astype(np.uint8).reshape(rows, w * ch)
    if depth == 16:
        return np.stack([px >> 8, px & 255], -1).astype(np.uint8).reshape(rows, w * ch * 2)
    bits = ((px.reshape(rows, w, 1) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(rows, w * depth)
    return np.packbits(bits, axis=1)                 # the last byte's low bits are zero


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_row(kind, cur, prev, bpp):
    cur, prev = cur.astype(np.int32), prev.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
    c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
    pred = {0: 0, 1: a, 2: prev, 3: (a + prev) // 2, 4: _paeth(a, prev, c)}[kind]
    return ((cur - pred) & 255).astype(np.uint8)


def passes_of(w, h, interlace):
    return ADAM7 if interlace else [(0, 0, 1, 1)]


def filtered_stream(px, depth, ctype, interlace, schedule) -> bytes:
    """schedule: a sequence of filters, cycled over the rows of each pass, or a callable (pass, row) -> filter"""
    h, w, ch = px.shape
    bits_pp = ch * depth
    bpp = max(1, bits_pp // 8)
    pick = schedule if callable(schedule) else (lambda ps, row: schedule[row % len(schedule)])
    out = bytearray()
    for ps, (x0, y0, dx, dy) in enumerate(passes_of(w, h, interlace)):
        sub = px[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        rows = pack_rows(sub, depth)
        prev = np.zeros(rows.shape[1], np.uint8)
        for r in range(rows.shape[0]):
            kind = pick(ps, r)
            out.append(kind)
            out += filter_row(kind, rows[r], prev, bpp).tobytes() if kind <= 4 else rows[r].tobytes()
            prev = rows[r]
    return bytes(out)


def palette(n=256, seed=5) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8).tobytes()


def assemble(w, h, ctype, depth, interlace, stream_z: bytes, plte=None, exif=None, idat_cuts=(), ihdr_interlace=None) -> bytes:
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace if ihdr_interlace is None else ihdr_interlace)
    out = SIG + chunk(b"IHDR", ihdr)
    if exif is not None:
        out += chunk(b"eXIf", exif)
    if plte is not None:
        out += chunk(b"PLTE", plte)
    cuts = [0] + [c for c in idat_cuts] + [len(stream_z)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", stream_z[a:b])
    return out + chunk(b"IEND", b"")


def make(w, h, ctype=2, depth=8, interlace=0, schedule=CYCLE, seed=1, px=None, plte=None, exif=None, idat_cuts=(), level=6) -> bytes:
    if px is None:
        px = samples(w, h, ctype, depth, seed)
    if ctype == 3 and plte is None:
        plte = palette(1 << depth)
    z = zlib.compress(filtered_stream(px, depth, ctype, interlace, schedule), level)
    return assemble(w, h, ctype, depth, interlace, z, plte, exif, idat_cuts)


def expected_rgb(px, ctype, depth, plte=None):
    """into_rgb8 of the samples: grey scaled by 255 / 85 / 17, 16 bit as (v + 128) / 257, alpha dropped, the palette"""
    v = px.astype(np.int64)
    if ctype == 3:
        return np.frombuffer(plte, np.uint8).reshape(-1, 3)[v[..., 0]]
    v8 = (v + 128) // 257 if depth == 16 else (v * (255 // ((1 << depth) - 1)) if depth < 8 else v)
    rgb = v8[..., [0, 0, 0]] if ctype in (0, 4) else v8[..., :3]
    return rgb.astype(np.uint8)


def exif_block(orientation, focal=None) -> bytes:
    """little-endian TIFF: IFD0 with Orientation and, with `focal`, an Exif sub-IFD holding FocalLengthIn35mmFilm"""
    n = 2 if focal is not None else 1
    ifd0 = struct.pack("<H", n) + struct.pack("<HHIHH", 0x0112, 3, 1, orientation, 0)
    sub_at = 8 + 2 + 12 * n + 4
    if focal is not None:
        ifd0 += struct.pack("<HHII", 0x8769, 4, 1, sub_at)
    ifd0 += struct.pack("<I", 0)
    out = b"II" + struct.pack("<HI", 42, 8) + ifd0
    if focal is not None:
        out += struct.pack("<H", 1) + struct.pack("<HHIHH", 0xA405, 3, 1, focal, 0) + struct.pack("<I", 0)
    return out


def with_exif(data: bytes, orientation, focal=None) -> bytes:
    """the file with an eXIf chunk behind IHDR (behind any it has: the last one counts)"""
    at = data.index(b"IDAT") - 4
    return data[:at] + chunk(b"eXIf", exif_block(orientation, focal)) + data[at:]


def all_pairs():
    """26 filters in which every ordered pair of the five follows each other once (an Euler tour of the complete digraph)"""
    edges = {a: list(range(5)) for a in range(5)}
    stack, tour = [0], []
    while stack:
        v = stack[-1]
        if edges[v]:
            stack.append(edges[v].pop())
        else:
            tour.append(stack.pop())
    tour.reverse()
    assert len(tour) == 26 and len({(a, b) for a, b in zip(tour, tour[1:])}) == 25
    return tuple(tour)


def _files():
    out = []

    def add(name, *a, **kw):
        out.append((name, lambda: make(*a, **kw)))

    # every (colour type, depth) pair, plain and Adam7; 33 pixels: row bit counts that are no multiple of 8, row byte
    # counts that are no multiple of 4
    for ctype, depth in TABLE:
        for il in (0, 1):
            add(f"t{ctype}d{depth}i{il}", 33, 17, ctype, depth, il, seed=ctype * 16 + depth)
    # filter schedules, at 3, 8 and 1 bytes of filter distance; 67 x 66: one row group and two rows
    for ctype, depth, tag in ((2, 8, "rgb8"), (6, 16, "rgba16"), (0, 1, "g1")):
        for k in range(5):
            add(f"{tag}-all{k}", 67, 66, ctype, depth, 0, (k,))
        add(f"{tag}-cycle-i", 67, 66, ctype, depth, 1, CYCLE)
        add(f"{tag}-pairs", 17, 31, ctype, depth, 0, all_pairs())
        for k in (2, 3, 4):
            add(f"{tag}-first{k}", 9, 9, ctype, depth, 1, (k, 0, 1))
    # shapes: no left or no upper neighbour, narrower than the skew, around a row group and a band, past the LDS tile
    for w, h in ((1, 1), (1, 70), (130, 1), (3, 2), (7, 9), (13, 5), (5, 70), (130, 3)):
        for il in (0, 1):
            add(f"s{w}x{h}i{il}", w, h, 2, 8, il, (4, 3, 4, 2, 1))
    for h in (GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1, BAND_ROWS - 1, BAND_ROWS, BAND_ROWS + 1):
        add(f"rows{h}", 9, h, 2, 8, 0, (4, 4, 3))
    add("rows-i", 5, 2 * BAND_ROWS + 3, 4, 8, 1, (3, 4))
    add("tile+1", TILE_BYTES + 1, 5, 0, 8, 0, (4, 3, 1))
    add("tile+1px", TILE_BYTES // 3 + 1, 70, 2, 8, 0, (4, 3))
    add("tile-exact", TILE_BYTES // 4, 66, 6, 8, 0, (4,))
    add("tiles", 300, 130, 2, 8, 0, (4, 3, 4, 4, 2, 3))          # five tiles, three row groups trailing each other
    add("tiles16", 150, 67, 6, 16, 0, (4, 3))
    # Adam7 with every subset of passes empty once
    for w in range(1, 10):
        for h in range(1, 10):
            add(f"a7-{w}x{h}", w, h, 2, 8, 1, (4, 3, 2, 1))
    # 16-bit samples around the rounding steps
    edge = np.array(EDGE16, np.uint16)
    for ctype in (0, 2, 4, 6):
        px = np.stack([np.roll(edge, c)[np.add.outer(np.arange(5), np.arange(11)) % 8] for c in range(CHANNELS[ctype])], -1)
        out.append((f"edge16c{ctype}", lambda px=px, ctype=ctype: make(11, 5, ctype, 16, 0, (0, 4, 3), px=px)))
    # eXIf: one file per orientation, with a focal length
    for o in range(1, 9):
        add(f"exif{o}", 13, 5, 2, 8, 0, CYCLE, exif=exif_block(o, 35))
    out.append(("exif-twice", lambda: with_exif(make(13, 5, exif=exif_block(3)), 6)))
    # several IDAT chunks: cut in the middle of a row, an empty one
    add("idat-split", 33, 17, 2, 8, 0, CYCLE, idat_cuts=(1, 40, 41, 41, 200), level=0)
    add("idat-split-i", 33, 17, 2, 16, 1, CYCLE, idat_cuts=(150, 150), level=0)
    return out


FILES = _files()


def _refused():
    def good_stream(w=9, h=7, ctype=2, depth=8, il=0, schedule=CYCLE):
        return filtered_stream(samples(w, h, ctype, depth), depth, ctype, il, schedule)

    def bad_filter():
        s = bytearray(good_stream())
        s[3 * (9 * 3 + 1)] = 5                                     # the filter byte of row 3
        return assemble(9, 7, 2, 8, 0, zlib.compress(bytes(s)))

    def short_palette():
        px = samples(9, 7, 3, 8)
        px[4, 4] = 200
        return make(9, 7, 3, 8, px=px % 201, plte=palette(200))     # 600 bytes: index 199 is the last whole entry

    def short_palette_edge():
        px = np.full((2, 2, 1), 3, np.uint16)
        return make(2, 2, 3, 2, px=px, plte=palette(4)[:11])        # 3 * 3 + 2 >= 11

    def truncated_stream():
        return assemble(9, 7, 2, 8, 0, zlib.compress(good_stream()[:-5]))

    def cut_deflate():
        return assemble(9, 7, 2, 8, 0, zlib.compress(good_stream())[:-9])

    def overlong_stream():
        return assemble(9, 7, 2, 8, 0, zlib.compress(good_stream() + b"\x00"))

    def wrong_adler():
        z = bytearray(zlib.compress(good_stream()))
        z[-1] ^= 0x55
        return assemble(9, 7, 2, 8, 0, bytes(z))

    def no_idat():
        return SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 7, 8, 2, 0, 0, 0)) + chunk(b"IEND", b"")

    def bad_pair():
        return assemble(9, 7, 2, 4, 0, zlib.compress(good_stream()))

    def bad_pair16():
        return assemble(9, 7, 3, 16, 0, zlib.compress(good_stream()), plte=palette())

    def bad_depth():
        return assemble(9, 7, 0, 3, 0, zlib.compress(good_stream()))

    def bad_ctype():
        return assemble(9, 7, 5, 8, 0, zlib.compress(good_stream()))

    def interlace2():
        return assemble(9, 7, 2, 8, 0, zlib.compress(good_stream()), ihdr_interlace=2)

    def truncated_chunk():
        data = make(9, 7)
        return data[:len(data) - 20]

    def two_defects():
        # a palette index out of range in row 1, a bad filter byte in row 3: the host meets the palette first
        px = samples(9, 7, 3, 8) % 100
        px[1, 2] = 250
        s = bytearray(filtered_stream(px, 8, 3, 0, (0,)))
        s[3 * 10] = 9
        return assemble(9, 7, 3, 8, 0, zlib.compress(bytes(s)), plte=palette(100))

    def two_defects_filter_first():
        px = samples(9, 7, 3, 8) % 100
        px[5, 2] = 250
        s = bytearray(filtered_stream(px, 8, 3, 0, (0,)))
        s[2 * 10] = 7
        return assemble(9, 7, 3, 8, 0, zlib.compress(bytes(s)), plte=palette(100))

    def bad_filter_and_adler():
        s = bytearray(good_stream())
        s[0] = 6
        z = bytearray(zlib.compress(bytes(s)))
        z[-2] ^= 1
        return assemble(9, 7, 2, 8, 0, bytes(z))

    inflate = "PNG data does not inflate to the image size"
    return [("bad-filter", bad_filter, "bad PNG filter"), ("short-plte", short_palette, "palette index out of range"),
            ("short-plte-edge", short_palette_edge, "palette index out of range"),
            ("short-stream", truncated_stream, inflate), ("cut-deflate", cut_deflate, inflate),
            ("long-stream", overlong_stream, inflate), ("adler", wrong_adler, inflate), ("no-idat", no_idat, inflate),
            ("pair-2-4", bad_pair, "does not go with colour type"), ("pair-3-16", bad_pair16, "does not go with colour type"),
            ("depth3", bad_depth, "bad PNG bit depth 3"), ("ctype5", bad_ctype, "bad PNG colour type"),
            ("interlace2", interlace2, "bad PNG interlace method"), ("cut-chunk", truncated_chunk, "truncated PNG chunk"),
            ("two-defects", two_defects, "palette index out of range"),
            ("two-defects-filter-first", two_defects_filter_first, "bad PNG filter"),
            ("filter-and-adler", bad_filter_and_adler, inflate)]


REFUSED = _refused()


def read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"P6" and parts[2] == b"255", parts[:3]
    w, h = (int(v) for v in parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def host_decode(data: bytes, tmp_path, oriented=False, name="f"):
    """(exit code, pixels or None, stderr) of the host decoder on `data`"""
    src, dst = str(tmp_path / (name + ".png")), str(tmp_path / (name + ".host.ppm"))
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([SELFTEST, "decode", src, dst] + (["oriented"] if oriented else []), capture_output=True, text=True)
    return r.returncode, (read_ppm(dst) if r.returncode == 0 else None), r.stderr
