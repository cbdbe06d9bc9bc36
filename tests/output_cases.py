"""Shapes and contents for the output back end, shared by tests/test_output_cases_cpu.py (every case ADMITTED from the C oracle
alone, no GPU) and tests/test_gpu_output_shapes.py (the HIP kernels against that oracle, array equality everywhere).  A plain
module: no test lives here.

Shapes are numpy [rows, cols].  The three consumers of a depth map index it in three ways:
  * the clamp and the colour map take it flat;
  * the stereogram's sampler reads data[cols * y + x] with x < rows, y < cols -- defined for rows >= cols only;
  * the mesh takes width = shape[0], height = shape[1] and reads data[y * width + x]: the buffer seen as [height][width].
A mesh map is therefore built in its MESH VIEW [height, width] = [cols, rows] (what is planted there has to be next to what the
mesh thinks its neighbours are) and handed over reshaped to (rows, cols)."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from oracle import output_oracle as OO

LO, HI = np.float32(1.0) / np.float32(250.0), np.float32(1.0) / np.float32(0.1)      # CLAMP_RANGE, output.rs:51


def _depth(shape, seed=0, kind="scene"):
    """inverse-depth-like maps: smooth background + a few nearer rectangles (discontinuities).  shape: n (an n x n map, the
    generator tests/test_gpu_output.py has always used, value for value) or (rows, cols)"""
    rows, cols = (shape, shape) if np.isscalar(shape) else shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, rows, dtype=np.float32), np.linspace(0, 1, cols, dtype=np.float32),
                         indexing="ij")
    d = 0.2 + 0.15 * np.sin(3 * xx + 2 * yy) + 0.1 * yy
    if kind == "scene":
        for _ in range(6):
            if rows == cols and rows >= 4:
                n = rows
                x0, y0 = rng.integers(0, n - n // 4, size=2)
                w, h = rng.integers(n // 16, n // 4, size=2)
            else:       # per axis; a degenerate axis (or a map below 4 x 4) still gets rectangles of one or two pixels
                x0, y0 = rng.integers(0, max(1, cols - cols // 4)), rng.integers(0, max(1, rows - rows // 4))
                w = rng.integers(max(1, cols // 16), max(2, cols // 4) + 1)
                h = rng.integers(max(1, rows // 16), max(2, rows // 4) + 1)
            d[y0:y0 + h, x0:x0 + w] += rng.uniform(0.2, 1.5)
        d += rng.normal(0, 0.002, size=d.shape).astype(np.float32)
    return np.ascontiguousarray(d.astype(np.float32))


def _frozen(a):
    a.setflags(write=False)
    return a


def _nan(negative=False, payload=0):
    return np.array([(0xffc00000 if negative else 0x7fc00000) | payload], np.uint32).view(np.float32)[0]


# ---- mesh ----------------------------------------------------------------------------------------------------------
#                shape        quads
MESH_SHAPES = [(2, 2),      # 1
               (2, 300),    # 299      qw = 1: every quad starts a row
               (300, 2),    # 299      qh = 1
               (5, 7),      # 24
               (4, 342),    # 1023     one short of a workgroup
               (3, 513),    # 1024     exactly one workgroup
               (26, 42),    # 1025     one quad in the second workgroup; qw = 25: row wraps inside a thread's 4 quads
               (131, 601),  # 78 000   77 workgroups: the look-back walks past one 64-lane window
               (601, 131)]  # 78 000   the other orientation
MESH_CONTENTS = ("scene", "border", "checker", "flat", "nan")
MESH_SEED = 7       # every shape's `scene` / `nan` / `border` map is admitted with this one seed


@dataclass(frozen=True)
class MeshCase:
    shape: Tuple[int, int]
    content: str

    @property
    def name(self):
        return f"{self.shape[0]}x{self.shape[1]}-{self.content}"

    @property
    def width(self):
        return self.shape[0]

    @property
    def height(self):
        return self.shape[1]

    @property
    def nquads(self):
        return (self.shape[0] - 1) * (self.shape[1] - 1)

    @property
    def border_spikes(self):
        """scene / nan from (26,42) upward: an unused vertex is planted in the last row and one in the last column"""
        return self.nquads >= 1025


MESH_CASES = [MeshCase(s, c) for s in MESH_SHAPES for c in MESH_CONTENTS]
MESH_BY_NAME = {c.name: c for c in MESH_CASES}
# the device file producers run on these three
MESH_FILE_CASES = ("26x42-scene", "131x601-scene", "5x7-checker")


def _scene_view(case):
    """The existing generator in the mesh view, with two plantings (all values inside [1/250, 10] before the clamp):
    a plateau over x >= w // 4, y >= h // 4 that reaches the last row and column (0.5 +- 0.05 %: everything in it is kept,
    whatever the size does to the background's slope), and vertices of twice that value, each of which loses all its
    triangles and stays unused: one at (w // 4, h // 4) and, from (26,42) upward, one in the last column and one in the last
    row.  Outside the plateau the background and its rectangles decide."""
    w, h = case.width, case.height
    rng = np.random.default_rng(MESH_SEED + 1000)
    v = _depth((h, w), seed=MESH_SEED).copy()
    x0, y0 = w // 4, h // 4
    v[y0:, x0:] = 0.5 * (1 + rng.uniform(-5e-4, 5e-4, size=(h - y0, w - x0))).astype(np.float32)
    spikes = [(x0, y0)]
    if case.border_spikes:
        spikes += [(w - 1, h // 2), (w // 2, h - 1)]
    for x, y in spikes:
        v[y, x] = 1.0
    return v, spikes


def mesh_nan_positions(case):
    """(x, y, negative) of the NaNs of a `nan` map: the planted unused vertex and, from 35 vertices on, two more inside, one in
    the last column, one in the last row and the corner (on a two-wide strip "inside" is the first column or row)"""
    w, h = case.width, case.height
    pos = [(w // 4, h // 4, False)]
    if w * h >= 35:
        pos += [(w // 2, h // 2, True), (w - 2, h - 2, False), (w - 1, h // 3, True), (w // 3, h - 1, False),
                (w - 1, h - 1, True)]
    return pos


@functools.lru_cache(maxsize=None)
def mesh_map(name):
    """The case's map as handed to the library: f32 [rows, cols] = [width, height], not yet clamped, read-only"""
    case = MESH_BY_NAME[name]
    w, h = case.width, case.height
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if case.content == "flat":
        v = np.full((h, w), 0.7, np.float32)
    elif case.content == "checker":
        v = np.where((xx + yy) % 2 == 0, 0.2, 0.4).astype(np.float32)
    elif case.content == "border":
        # last row and last column at twice their neighbours (the corner at twice ITS neighbours, which are border vertices)
        rng = np.random.default_rng(MESH_SEED + 2000)
        v = (0.5 * (1 + rng.uniform(-5e-4, 5e-4, size=(h, w)))).astype(np.float32)
        v[h - 1, :] = 2 * v[h - 2, :]
        v[:, w - 1] = 2 * v[:, w - 2]
        v[h - 1, w - 1] = 4 * v[h - 2, w - 2]
    else:
        v, _ = _scene_view(case)
        if case.content == "nan":
            for x, y, neg in mesh_nan_positions(case):
                v[y, x] = _nan(neg)
    assert v.shape == (h, w) and v.dtype == np.float32
    assert np.all((v[~np.isnan(v)] >= LO) & (v[~np.isnan(v)] <= HI))      # nothing planted leaves the clamp range
    return _frozen(np.ascontiguousarray(v).reshape(w, h))


@functools.lru_cache(maxsize=None)
def mesh_oracle(name):
    """(clamped map [rows, cols], vertex_index, nverts, faces): the oracle's, computed once, read-only"""
    od, _, _ = OO.clamp_minmax(mesh_map(name))
    vi, nv, faces = OO.mesh_index(od)
    return _frozen(od), _frozen(vi), nv, _frozen(faces)


# ---- stereogram -------------------------------------------------------------------------------------------------------
STEREO_MAPS = {                      # name: (shape, seed, NaN pixel or None)
    "96x40": ((96, 40), 53, None),               # seed 53: the first from 21 on that admits the narrow range below
    "300x2": ((300, 2), 22, None),
    "1026x3": ((1026, 3), 23, None),
    "64x64": ((64, 64), 24, None),               # the control
    "96x40-nan": ((96, 40), 53, (50, 17)),
}
STEREO_WIDE = {"40x96": ((40, 96), 31), "2x300": ((2, 300), 32), "3x1026": ((3, 1026), 33)}   # refused: cols > rows
STEREO_SIZES = [(1, 1), (255, 3), (256, 3), (257, 3), (511, 2), (513, 2), (70, 1), (70, 200), (16384, 2)]   # (out_w, out_h)
AMP_BIG, AMP_ZERO = 0.6, 0.0005                 # pattern_width > out_w; pattern_width == 0 (out_w < 500)
NOISE_SEED = 99


@dataclass(frozen=True)
class StereoCase:
    map: str
    out_w: int
    out_h: int
    amplitude: float
    percentiles: Optional[Tuple[float, float]] = None      # the caller's [min_depth, max_depth], of the clamped map

    @property
    def name(self):
        p = "" if self.percentiles is None else f"-p{self.percentiles[0]:g}-{self.percentiles[1]:g}"
        return f"{self.map}-{self.out_w}x{self.out_h}-a{self.amplitude:g}{p}"


def _stereo_table():
    cases = []
    for name in STEREO_MAPS:
        cases += [StereoCase(name, w, h, 1.0 / 16.0) for w, h in STEREO_SIZES]
        cases += [StereoCase(name, w, h, 0.125) for w, h in ((257, 3), (70, 200), (16384, 2))]
        cases += [StereoCase(name, w, h, AMP_BIG) for w, h in ((1, 1), (257, 3), (70, 200))]
        cases += [StereoCase(name, w, h, AMP_ZERO) for w, h in ((1, 1), (256, 3), (257, 3), (70, 200))]
    return cases


STEREO_CASES = _stereo_table()
# A range narrower than the data: pixels beyond max_depth shift by more than pattern_width and refer FORWARD (the source
# index is > x), which only a caller-supplied range can do.  The percentiles are the 30th / 70th for both.  On (96,40) the seed
# of the map moved instead: with seeds 21 - 52 a near rectangle at the right-hand edge sends a source index past out_w (the
# oracle's -1) at 30 / 70, and with seed 21 at every pair from there out to 10.75 / 89.25, beyond which nothing refers forward.
NARROW_CASES = [StereoCase("96x40", 257, 3, 1.0 / 16.0, (30.0, 70.0)),
                StereoCase("64x64", 513, 2, 1.0 / 16.0, (30.0, 70.0))]
STEREO_BY_NAME = {c.name: c for c in STEREO_CASES + NARROW_CASES}


@functools.lru_cache(maxsize=None)
def stereo_map(name):
    """(clamped map, min, max) of a tall, square or wide stereogram map -- the oracle's clamp, read-only"""
    if name in STEREO_WIDE:
        shape, seed = STEREO_WIDE[name]
        nan_at = None
    else:
        shape, seed, nan_at = STEREO_MAPS[name]
    d = _depth(shape, seed=seed)
    if nan_at is not None:
        d[nan_at] = np.nan
    od, mn, mx = OO.clamp_minmax(d)
    return _frozen(od), mn, mx


@functools.lru_cache(maxsize=None)
def stereo_noise(out_w, out_h):
    return _frozen(np.random.default_rng(NOISE_SEED).integers(0, 256, size=(out_h, out_w, 3), dtype=np.uint8))


def stereo_range(case):
    """the [min_depth, max_depth] the case passes: the map's own, or the two percentiles of its clamped values"""
    od, mn, mx = stereo_map(case.map)
    if case.percentiles is None:
        return mn, mx
    lo, hi = np.percentile(od[~np.isnan(od)].astype(np.float64), case.percentiles)
    return float(np.float32(lo)), float(np.float32(hi))


@functools.lru_cache(maxsize=None)
def stereo_oracle(name):
    """(rc, out, forward, forward_strict) of OO.stereogram_counted for the case, computed once, read-only"""
    case = STEREO_BY_NAME[name]
    od, _, _ = stereo_map(case.map)
    mn, mx = stereo_range(case)
    rc, out, fwd, strict = OO.stereogram_counted(od, mn, mx, case.out_w, case.out_h, case.amplitude,
                                                 stereo_noise(case.out_w, case.out_h))
    return rc, (None if out is None else _frozen(out)), fwd, strict


def pattern_width(out_w, amplitude):
    """output.rs:160-161 in f32"""
    a = np.float32(amplitude)
    v = np.float32(np.float32(np.float32(out_w) * a) * np.float32(2.0)) + a
    r = np.float32(np.trunc(v + np.copysign(np.float32(0.5), v))) if np.isfinite(v) else v
    return max(0, int(r))


# ---- clamp -------------------------------------------------------------------------------------------------------------
CLAMP_COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 1025, 4099, 512 * 256 * 16 + 3]
CLAMP_CONTENTS = ("salted", "inner")
CLAMP_SPECIALS = np.concatenate([
    np.array([0x7fc00000, 0xffc00000, 0x7fc12345, 0xffc00001], np.uint32).view(np.float32),   # NaN, -NaN, payloads
    np.array([np.inf, -np.inf, 0.0, -0.0, -1.0, 1e-40], np.float32),                            # 1e-40: a subnormal
    np.array([LO, HI, np.nextafter(LO, np.float32(0)), np.nextafter(LO, np.float32(1)),
              np.nextafter(HI, np.float32(0)), np.nextafter(HI, np.float32(100))], np.float32)])


@functools.lru_cache(maxsize=None)
def clamp_case(count, content):
    """f32 [count], read-only.
    salted: log-uniform values in [1e-4, 1e2] with CLAMP_SPECIALS at random places -- as many as leave one ordinary value, in an
        order that rotates with the count, so that the small counts see different ones; the odd counts from 3 on have a NaN at
        index 0; the single element is the value just below 1/250.
    inner: log-uniform values in [0.01, 5], nothing leaves the clamp range, so (min, max) are the data's own and sit anywhere,
        the scalar tail included: from 5 elements on the smallest value (0.007) is planted in the last element and the largest
        (7.5) in the one before it; NaNs of both signs at random places and (odd counts from 3 on) at index 0."""
    rng = np.random.default_rng(1000 + count % 9973 + (0 if content == "salted" else 50000))
    if content == "salted":
        d = np.exp(rng.uniform(np.log(1e-4), np.log(1e2), size=count)).astype(np.float32)
        k = min(count - 1, len(CLAMP_SPECIALS))
        specials = np.roll(CLAMP_SPECIALS, -(count % len(CLAMP_SPECIALS)))[:k]
        places = rng.permutation(count)[:k]
        d[places] = specials
        if count == 1:
            d[0] = np.nextafter(LO, np.float32(0))
        if count >= 3 and count % 2 == 1:
            d[0] = _nan()
    else:
        d = np.exp(rng.uniform(np.log(0.01), np.log(5.0), size=count)).astype(np.float32)
        k = min(count // 3, 6)
        d[rng.permutation(count)[:k]] = [_nan(i % 2 == 1, i) for i in range(k)]
        if count >= 5:
            d[count - 1], d[count - 2] = np.float32(0.007), np.float32(7.5)
        if count >= 3 and count % 2 == 1:
            d[0] = _nan(True)
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def clamp_oracle(count, content):
    od, mn, mx = OO.clamp_minmax(clamp_case(count, content))
    return _frozen(od), mn, mx


# ---- colour map ------------------------------------------------------------------------------------------------------
COLOUR_SHAPES = [(96, 40), (40, 96), (1, 5)]
COLOUR_CONTENTS = ("scene", "flat", "nan")


@functools.lru_cache(maxsize=None)
def colour_map(shape, content):
    """f32 [rows, cols] before the clamp, read-only; flat: max == min, so every t is 0 / 0"""
    if content == "flat":
        return _frozen(np.full(shape, 0.7, np.float32))
    d = _depth(shape, seed=40 + shape[0])
    if content == "nan":
        flat = d.reshape(-1)
        flat[[0, flat.size // 2, flat.size - 1]] = [_nan(), _nan(True), _nan(False, 7)]
    return _frozen(d)
