"""CPU tests of the Lanczos3 resampler's host half: me_op_lanczos3_table, the per-axis table the kernels of
csrc/resample.hip run on (reference reconstruction.rs:107-113, output.rs:133-137, output.rs:206-218: the `image`
crate's Lanczos3 sampler, restated in oracle/image_oracle.c).  The table is built on the host, so all of this runs
without a GPU; the kernels are held to the oracle in test_gpu_resample.py."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def image_oracle():
    from oracle import output_oracle
    output_oracle.build()
    return C.CDLL(os.path.join(ROOT, "oracle", "_build", "libimage_oracle.so"))


def oracle_resize(img, nw, nh):
    h, w, _ = img.shape
    a = np.ascontiguousarray(img)
    want = np.empty((nh, nw, 3), np.uint8)
    assert image_oracle().oracle_resize_lanczos3_rgb8(C.c_void_p(a.ctypes.data), C.c_int64(w), C.c_int64(h),
                                                      C.c_void_p(want.ctypes.data), C.c_int64(nw), C.c_int64(nh)) == 0
    return want


def table(lib, len_in, len_out):
    need = lib.me_op_lanczos3_table(len_in, len_out, None, None, None, 0)
    assert need > 0
    left, count = np.full(len_out, -7, np.int32), np.full(len_out, -7, np.int32)
    weights = np.full(need, np.nan, np.float32)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    got = lib.me_op_lanczos3_table(len_in, len_out, left.ctypes.data_as(i32p), count.ctypes.data_as(i32p),
                                   weights.ctypes.data_as(f32p), need)
    assert got == need
    return left, count, weights


def closed_form(len_in, len_out):
    """left / right of the oracle's header comment, every operation rounded to f32"""
    ratio = F(len_in) / F(len_out)
    sratio = max(ratio, F(1))
    support = F(3) * sratio
    left, count = [], []
    for o in range(len_out):
        center = (F(o) + F(0.5)) * ratio
        lo = min(max(int(np.floor(center - support)), 0), len_in - 1)
        hi = min(max(int(np.ceil(center + support)), lo + 1), len_in)
        left.append(lo), count.append(hi - lo)
    return np.array(left, np.int32), np.array(count, np.int32)


@pytest.mark.parametrize("pair", [(3024, 1536), (1536, 4032), (7, 3), (1, 5), (40, 1), (257, 256), (100, 100)])
def test_table_spans_and_normalisation(lib, pair):
    len_in, len_out = pair
    left, count, weights = table(lib, len_in, len_out)
    want_left, want_count = closed_form(len_in, len_out)
    assert np.array_equal(left, want_left) and np.array_equal(count, want_count)
    assert weights.size == int(count.sum()) and np.isfinite(weights).all()
    sums = np.add.reduceat(weights.astype(np.float64), np.concatenate([[0], np.cumsum(count)[:-1]]))
    worst = float(np.abs(sums - 1.0).max())
    print(f"{len_in} -> {len_out}: counts up to {count.max()}, |sum - 1| <= {worst:.3g}")
    assert worst <= 1e-6


def test_table_capacity_and_bad_arguments(lib):
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    need = lib.me_op_lanczos3_table(40, 30, None, None, None, 0)
    left, count = np.full(30, -7, np.int32), np.full(30, -7, np.int32)
    weights = np.full(need, 123.0, np.float32)
    args = (left.ctypes.data_as(i32p), count.ctypes.data_as(i32p), weights.ctypes.data_as(f32p))
    assert lib.me_op_lanczos3_table(40, 30, *args, need - 1) == need          # too small: the count, nothing written
    assert (left == -7).all() and (count == -7).all() and (weights == 123.0).all()
    assert lib.me_op_lanczos3_table(40, 30, *args, need) == need and (count > 0).all()
    for bad in [(0, 5), (5, 0), (-1, 5), (5, -3), (1 << 20, 5), (5, 1 << 20)]:
        assert lib.me_op_lanczos3_table(*bad, *args, need) < 0, bad
    assert lib.me_op_lanczos3_table(40, 30, None, None, None, need) < 0       # room promised, nowhere to write


def apply_tables(lib, img, nw, nh):
    """the two passes of imageops::resize with the library's tables, every operation an np.float32 scalar, in the
    oracle's order: vertical into an unclamped f32 intermediate, horizontal, clamp, round half away from zero"""
    h, w, _ = img.shape
    lv, cv, wv = table(lib, h, nh)
    lh, ch, wh = table(lib, w, nw)
    ov, oh = np.concatenate([[0], np.cumsum(cv)]), np.concatenate([[0], np.cumsum(ch)])
    src = img.astype(np.float32)
    mid = np.zeros((nh, w, 3), np.float32)
    for o in range(nh):
        for x in range(w):
            for c in range(3):
                t = F(0)
                for i in range(cv[o]):
                    t = F(t + F(src[lv[o] + i, x, c] * wv[ov[o] + i]))
                mid[o, x, c] = t
    out = np.zeros((nh, nw, 3), np.uint8)
    for y in range(nh):
        for o in range(nw):
            for c in range(3):
                t = F(0)
                for i in range(ch[o]):
                    t = F(t + F(mid[y, lh[o] + i, c] * wh[oh[o] + i]))
                t = min(max(t, F(0)), F(255))
                out[y, o, c] = int(np.floor(np.float64(t) + 0.5))    # exact in f64; t >= 0, so half goes up
    return out


@pytest.mark.parametrize("case", [((40, 30), (17, 23)), ((9, 11), (31, 29)), ((1, 7), (5, 3)), ((40, 30), (1, 1)),
                                  ((64, 8), (1, 8))])
def test_table_is_the_oracles(lib, case):
    """The host-side sine and the no-contraction rule, before a GPU is involved: the library's two tables applied in
    plain f32 arithmetic give the oracle's bytes."""
    (w, h), (nw, nh) = case
    rng = np.random.default_rng(w * 31 + nh)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[rng.integers(0, h, 8), rng.integers(0, w, 8)] = rng.integers(0, 2, (8, 1), dtype=np.uint8) * 255
    assert np.array_equal(apply_tables(lib, img, nw, nh), oracle_resize(img, nw, nh))
