"""Pictures and parameters shared by the JPEG encoder tests (tests/test_jpeg_encode_cpu.py, tests/test_gpu_jpeg_encode.py):
the shape list, the three named pictures with the conditions that make them worth encoding, and the seam picture.  Every
picture is uint8 [h, w, 3] and a pure function of its arguments."""
import functools

import numpy as np

import jpeg_encode_ref as R

SHAPES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (37, 53), (2, 70), (47, 3), (64, 48)]   # (width, height)
QUALITIES = (1, 25, 75, 95, 100)
SUBSAMPLINGS = (0, 1, 2)


def noise(w, h, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40) % 256, (xx + yy * 2) % 256], -1).astype(np.uint8)


def shape_picture(w, h):
    """noise in the left half, a ramp in the right one: long and short zero runs in one file"""
    rgb = noise(w, h, seed=w * 131 + h)
    rgb[:, w // 2:] = smooth(w, h)[:, w // 2:]
    return rgb


def checker():
    """40 x 72, 120 everywhere and +-60 on a one-pixel checkerboard in the blocks with (bx + by) % 3 == 0: at quality 10 the
    checkerboard's energy sits at the far end of the zigzag, behind runs of more than 48 zeros"""
    h, w = 72, 40
    yy, xx = np.mgrid[0:h, 0:w]
    on = ((xx // 8 + yy // 8) % 3) == 0
    v = 120 + np.where(on, np.where((xx + yy) % 2 == 0, 60, -60), 0)
    return np.repeat(v[..., None], 3, axis=2).astype(np.uint8)


def flat():
    return np.full((80, 64, 3), 77, np.uint8)


NAMED = [("checker", checker, 10), ("noise", lambda: noise(96, 136, seed=7), 100), ("flat", flat, 75)]   # name, maker, quality
SEAMS = (200, 264)   # noise at quality 100: 825 blocks at 4:4:4, more than one workgroup of every kernel


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, quality, subsampling):
    """(file, counters) of the yardstick, computed once per case and shared"""
    rgb = picture(kind, w, h)
    return R.encode(rgb, quality, subsampling)


def picture(kind, w=0, h=0):
    if kind == "shape":
        return shape_picture(w, h)
    if kind == "seams":
        return noise(SEAMS[0], SEAMS[1], seed=3)
    return dict((n, mk) for n, mk, _ in NAMED)[kind]()


def cases():
    """every (kind, w, h, quality, subsampling) of the byte-equality tests"""
    out = [("shape", w, h, q, s) for (w, h) in SHAPES for q in QUALITIES for s in SUBSAMPLINGS]
    for name, make, q in NAMED:
        hh, ww = make().shape[:2]
        out += [(name, ww, hh, q, s) for s in SUBSAMPLINGS]
    return out
