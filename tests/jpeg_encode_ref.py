"""The yardstick of the JPEG encoder tests: libjpeg's baseline path (optimize=False) restated in numpy -- jccolor.c, the
h2v1 / h2v2 down-samplers with libjpeg's edge order, jfdctint.c, the integer quantiser, the dummy blocks of partial MCUs,
the Annex K tables and the bit stuffing.  encode(rgb, quality, subsampling) returns the file's bytes and counters that say
what the picture exercised: blocks, dummy blocks, ZRL symbols, the longest zero run and the stuffed bytes."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
          47, 55, 62, 63]
BASE_Q = [
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
     95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
     99, 99] + [99] * 32,
]
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = [list(range(12)), list(range(12))]
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]]
_TAIL = [r << 4 | s for r in range(16) for s in range(1, 11)]


def _ac_vals(head):
    return head + [v for v in _TAIL if v not in head]


AC_VALS = [
    _ac_vals([0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
              0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
              0x82, 0x09, 0x0a]),
    _ac_vals([0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
              0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
              0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a]),
]


def _codes(bits, vals):
    """symbol -> (code, length) of a canonical table"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
AC_CODES = [_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def quant_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((np.array(b, np.int64) * scale + 50) // 100, 1, 255) for b in BASE_Q]


def _fix(x):
    return int(x * 65536 + 0.5)


def _ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _planes(rgb, hs, vs):
    h, w = rgb.shape[:2]
    y, cb, cr = _ycc(rgb)
    out = [_pad(y, -(-h // 8) * 8, -(-w // 8) * 8)]
    for p in (cb, cr):
        cw, ch = -(-w // hs), -(-h // vs)
        wb, hb = -(-cw // 8), -(-ch // 8)
        if hs == 1:
            out.append(_pad(p, hb * 8, wb * 8))
            continue
        p = _pad(p, -(-h // vs) * vs, wb * 8 * 2)       # to the right in full, downward only to a multiple of vs
        bias = np.arange(wb * 8) & 1
        if vs == 2:
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + bias) >> 2
        else:
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append(_pad(p, hb * 8, wb * 8))             # the down-sampled last row, downward
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """jfdctint.c on the last axis of d [..., 8]"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    o[0] = (t10 + t11) * 4 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) * 4 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _blocks(plane, q):
    """plane [hb*8, wb*8] -> quantised coefficients [hb, wb, 64], natural order"""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128
    b = _fdct_pass(b, True)
    b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2).reshape(hb, wb, 64)
    qv = q << 3
    return np.sign(b) * ((np.abs(b) + (qv >> 1)) // qv)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def header(w, h, quality, hs, vs):
    q = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(q[t][ZIGZAG[k]]) for k in range(64))
    out += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, bits, vals in ((0x00, DC_BITS[0], DC_VALS[0]), (0x10, AC_BITS[0], AC_VALS[0]),
                           (0x01, DC_BITS[1], DC_VALS[1]), (0x11, AC_BITS[1], AC_VALS[1])):
        n = 19 + len(vals)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, tc]) + bytes(bits) + bytes(vals)
    return bytes(out + b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")


def encode(rgb, quality=75, subsampling=2):
    """rgb uint8 [h, w, 3] -> (file bytes, counters)"""
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    hs, vs = ((1, 1), (2, 1), (2, 2))[subsampling]
    q = quant_tables(quality)
    planes = _planes(rgb, hs, vs)
    coef = [_blocks(planes[0], q[0]), _blocks(planes[1], q[1]), _blocks(planes[2], q[1])]
    hb, wb = coef[0].shape[:2]
    bits = _Bits()
    pred = [0, 0, 0]
    stats = {"blocks": 0, "dummy_blocks": 0, "zrl": 0, "longest_run": 0, "stuffed": 0}
    for my in range(-(-h // (8 * vs))):
        for mx in range(-(-w // (8 * hs))):
            units = [(0, mx * hs + x, my * vs + y) for y in range(vs) for x in range(hs)] + [(1, mx, my), (2, mx, my)]
            last = None
            for c, bx, by in units:
                stats["blocks"] += 1
                if c == 0 and (bx >= wb or by >= hb):
                    stats["dummy_blocks"] += 1
                    blk = np.zeros(64, np.int64)
                    blk[0] = last[0]
                else:
                    blk = coef[c][by, bx]
                last = blk
                t = 0 if c == 0 else 1
                n, mag = _magnitude(int(blk[0]) - pred[c])
                pred[c] = int(blk[0])
                bits.put(*DC_CODES[t][n])
                bits.put(mag, n)
                run = 0
                for k in range(1, 64):
                    v = int(blk[ZIGZAG[k]])
                    if v == 0:
                        run += 1
                        continue
                    stats["longest_run"] = max(stats["longest_run"], run)
                    while run > 15:
                        bits.put(*AC_CODES[t][0xf0])
                        stats["zrl"] += 1
                        run -= 16
                    n, mag = _magnitude(v)
                    bits.put(*AC_CODES[t][run << 4 | n])
                    bits.put(mag, n)
                    run = 0
                if run:
                    bits.put(*AC_CODES[t][0x00])
    scan = bits.finish()
    stats["stuffed"] = scan.count(b"\xff")
    return header(w, h, quality, hs, vs) + scan.replace(b"\xff", b"\xff\x00") + b"\xff\xd9", stats
