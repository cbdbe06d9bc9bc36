"""GPU test of the photo front end with both formats on one context (csrc/input_api.hip): JPEG and PNG decodes queued
alternately with no synchronise between them -- each format has its own pinned staging buffer and its own timing marks,
and a file one format refuses leaves the other's decodes alone.  The per-format suites (test_gpu_jpeg.py,
test_gpu_png_decode.py) cannot see any of that.  Every comparison is np.array_equal against the host decoders' bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from util import ctx_for, ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_files as J  # noqa: E402
import png_files as P  # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG = 1


@pytest.fixture(scope="module")
def ctx():
    return ctx_for("tiny", "f16")         # a context is enough: no weights are loaded for a decode


def host(ctx, kind, data, orientation=1):
    """the host decoder's pixels from inside the library, then apply_orientation (restated, held to host_selftest's by
    the CPU tests)"""
    w, h, _, _ = (ctx.jpeg_info if kind == "jpeg" else ctx.png_info)(data)
    out = np.empty((h, w, 3), np.uint8)
    decode = ctx.lib.me_op_jpeg_decode_host if kind == "jpeg" else ctx.lib.me_op_png_decode_host
    assert decode(data, len(data), C.c_void_p(out.ctypes.data), w, h) == 0
    return np.ascontiguousarray(P.orient(out, orientation))


def destinations(wants):
    dsts = [torch.full(want.shape, 7, dtype=torch.uint8, device="cuda") for want in wants]
    torch.cuda.synchronize()              # the fills are torch's; from here on nothing synchronises but the library
    return dsts


def queue(ctx, kind, data, orientation, dst):
    """one decode into a device destination, left on the stream"""
    decode = ctx.lib.me_jpeg_decode_rgb8 if kind == "jpeg" else ctx.lib.me_png_decode_rgb8
    return decode(ctx.handle, data, len(data), orientation, ptr(dst), dst.shape[1], dst.shape[0])


def test_formats_interleaved_on_one_context(ctx):
    """A small JPEG, a PNG turned by orientation 6, a larger JPEG (the JPEG staging buffer grows while uploads are pending)
    and a palette PNG (its decode synchronises), each into its own device destination."""
    files = dict(P.FILES)
    jobs = [("jpeg", J.plain(203, 111, 0, True, 70), 1), ("png", files["tiles"](), 6),
            ("jpeg", J.plain(517, 333, 2, False, 90), 1), ("png", files["t3d8i1"](), 1)]
    wants = [host(ctx, kind, data, o) for kind, data, o in jobs]
    dsts = destinations(wants)
    lib, hd = ctx.lib, ctx.handle
    for (kind, data, o), dst in zip(jobs, dsts):                   # no synchronise between the calls
        assert queue(ctx, kind, data, o, dst) == 0, lib.me_last_error(hd)
    assert lib.me_ctx_synchronize(hd) == 0
    for (kind, _, o), want, dst in zip(jobs, wants, dsts):
        assert np.array_equal(dst.cpu().numpy(), want), (kind, want.shape, o)
    jpeg_ms, png_ms = ctx.last_jpeg_timing(), ctx.last_png_timing()
    for ms in (jpeg_ms, png_ms):
        assert len(ms) == 5 and all(v >= 0 for v in ms) and ms[4] == 0    # device destinations: no download leg
    # one more JPEG decode, into a host array: its report has a download leg, the PNG report still tells of the last PNG
    assert np.array_equal(ctx.decode_jpeg(jobs[0][1]), wants[0])
    assert ctx.last_jpeg_timing()[4] > 0
    assert ctx.last_png_timing() == png_ms


def test_a_refusal_of_one_format_between_two_decodes_of_the_other(ctx):
    files = dict(P.FILES)
    lib, hd = ctx.lib, ctx.handle
    small = np.zeros((32, 32, 3), np.uint8)
    png_a, png_b = files["tiles"](), files["t2d8i0"]()
    want_a, want_b = host(ctx, "png", png_a), host(ctx, "png", png_b, 3)
    dst_a, dst_b = destinations((want_a, want_b))
    rc_a = queue(ctx, "png", png_a, 1, dst_a)
    cmyk = J.cmyk()
    assert lib.me_jpeg_decode_rgb8(hd, cmyk, len(cmyk), 1, C.c_void_p(small.ctypes.data), 32, 32) == BAD_ARG
    assert b"4 components" in lib.me_last_error(hd)
    rc_b = queue(ctx, "png", png_b, 3, dst_b)
    assert (rc_a, rc_b) == (0, 0) and lib.me_ctx_synchronize(hd) == 0
    assert np.array_equal(dst_a.cpu().numpy(), want_a) and np.array_equal(dst_b.cpu().numpy(), want_b)

    jpeg_a, jpeg_b = J.plain(203, 111, 0, True, 70), J.plain(64, 48)
    want_a, want_b = host(ctx, "jpeg", jpeg_a), host(ctx, "jpeg", jpeg_b, 8)
    dst_a, dst_b = destinations((want_a, want_b))
    rc_a = queue(ctx, "jpeg", jpeg_a, 1, dst_a)
    bad = dict((name, make) for name, make, _ in P.REFUSED)["bad-filter"]()
    assert lib.me_png_decode_rgb8(hd, bad, len(bad), 1, C.c_void_p(small.ctypes.data), 9, 7) == BAD_ARG
    assert b"bad PNG filter" in lib.me_last_error(hd)
    rc_b = queue(ctx, "jpeg", jpeg_b, 8, dst_b)
    assert (rc_a, rc_b) == (0, 0) and lib.me_ctx_synchronize(hd) == 0
    assert np.array_equal(dst_a.cpu().numpy(), want_a) and np.array_equal(dst_b.cpu().numpy(), want_b)
