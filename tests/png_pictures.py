"""The test pictures of the PNG encoder tests and of tools/bench_png.py: seeded, generated, nothing read from outside
the repository.  All are uint8 [h, w, 3]."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def viridis_lut() -> np.ndarray:
    """The colour table of include/me_viridis_lut.h as uint8 [n, 3] (rounded from its floats)."""
    text = open(os.path.join(ROOT, "include", "me_viridis_lut.h")).read()
    body = text[text.index("{", text.index("=")):]
    vals = [float(v.rstrip("fF")) for v in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?[fF]?|\b\d+\b", body)]
    vals = np.array(vals[: len(vals) // 3 * 3], np.float64).reshape(-1, 3)
    if vals.max() <= 1.0:
        vals = vals * 255.0
    return np.clip(np.round(vals), 0, 255).astype(np.uint8)


def inverse_depth_field(size=1536, seed=3) -> np.ndarray:
    """A smooth synthetic inverse-depth field [size, size] f32 with a step edge and 0.2 % Gaussian noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64) / size
    d = 0.05 + 0.6 * np.exp(-((x - 0.45) ** 2 + (y - 0.55) ** 2) / 0.08) + 0.15 * np.sin(3.0 * x + 2.0 * y) ** 2
    d[(x > 0.7) & (y > 0.2) & (y < 0.8)] += 0.8                       # the step edge
    d *= 1.0 + 0.002 * rng.standard_normal(d.shape)
    return np.clip(d, 1.0 / 250.0, 10.0).astype(np.float32)


def depth_picture(size=1536, seed=3) -> np.ndarray:
    """That field through the viridis table (numpy restatement: nearest table entry)."""
    d = inverse_depth_field(size, seed).astype(np.float64)
    lut = viridis_lut()
    t = (d - d.min()) / (d.max() - d.min())
    return lut[np.clip(np.round(t * (len(lut) - 1)).astype(np.int64), 0, len(lut) - 1)]


def stereogram_like(h, w, seed=5, pattern=None) -> np.ndarray:
    """numpy restatement of an autostereogram's structure: a random strip of `pattern` pixels repeated along each row,
    the repeat distance shortened by up to 1/16 where the depth field is near."""
    rng = np.random.default_rng(seed)
    pattern = pattern or max(8, w // 8)
    size = 256
    d = inverse_depth_field(size, seed)
    d = (d - d.min()) / (d.max() - d.min())
    ys = np.arange(h) * size // h
    xs = np.arange(w) * size // w
    shift = np.round(d[np.ix_(ys, xs)] * (pattern / 16.0)).astype(np.int64)
    out = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rows = np.arange(h)
    for x in range(pattern, w):
        out[rows, x] = out[rows, x - pattern + shift[:, x]]
    return out


def noise_picture(h, w, seed=7) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat_picture(h, w) -> np.ndarray:
    return np.zeros((h, w, 3), np.uint8)


def checkerboard(h, w) -> np.ndarray:
    """Two colours in squares of one pixel."""
    out = np.empty((h, w, 3), np.uint8)
    odd = (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)
    out[~odd] = (12, 200, 90)
    out[odd] = (240, 33, 160)
    return out


def alternating_rows(seed=11) -> np.ndarray:
    """Two random rows of 13333 pixels alternating over 8 rows: whatever filter a row gets, the stream repeats only at
    80 KB, beyond deflate's 32 KiB window."""
    two = np.random.default_rng(seed).integers(0, 256, (2, 13333, 3), dtype=np.uint8)
    return np.ascontiguousarray(two[[0, 1] * 4])


def around_chunks(chunk=65536, max_dim=16384):
    """{delta: (h, w)} for delta = -1, 0, +1: pictures whose filtered stream h * (3w + 1) is one byte less than, exactly,
    and one byte more than a whole number of chunks -- the smallest such found by search."""
    found = {}
    for delta in (-1, 0, 1):
        for n in range(1, 8):
            target = chunk * n + delta
            for h in range(1, 4000):
                if target % h == 0 and (target // h - 1) % 3 == 0 and 0 < (target // h - 1) // 3 <= max_dim:
                    found.setdefault(delta, (h, (target // h - 1) // 3))
    return found
