"""The prefix sums of csrc/scan.h on the GPU (-m gpu) through me_op_exclusive_scan_u32, against numpy.cumsum in uint64:
form 0 is the one-workgroup scan the OBJ text runs (1024 threads, a slice per thread), form 1 the two-level scan the
JPEG encoder runs (256 per workgroup, then one workgroup over the aggregates).  Sizes around one workgroup, around one
element per thread of the one-workgroup kernel and, in form 1, around 65 536 = 256 * 256, where the carry's threads
begin to walk more than one aggregate; sums that pass 2^32; a base above 2^32; the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from util import ctx_for

pytestmark = pytest.mark.gpu
SIZES = {0: (0, 1, 1023, 1024, 1025, 3077), 1: (1, 255, 256, 257, 65536, 65537, 131075)}
BASES = (0, (1 << 32) + 12345)
GUARD = 0xA5A5A5A5A5A5A5A5
ME_ERR_BAD_ARG = 1


def _ctx():
    return ctx_for("tiny", "f16")


@functools.lru_cache(maxsize=None)
def _case(n, values):
    """(counts, exclusive sums with the total at [n]) in uint64, computed once and read-only"""
    if values == "random":
        counts = np.random.default_rng(1000 + n).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    else:
        counts = np.zeros(n, np.uint32)
        if values == "last" and n:
            counts[-1] = 0xFFFFFFFF
    want = np.zeros(n + 1, np.uint64)
    np.cumsum(counts.astype(np.uint64), out=want[1:])
    counts.setflags(write=False)
    want.setflags(write=False)
    return counts, want


def _scan(ctx, counts, base, form):
    """the entry on device tensors -> offsets[n + 1], with a guard word behind them checked"""
    n = len(counts)
    dc = torch.from_numpy(counts.view(np.int32).copy()).cuda()
    out = torch.from_numpy(np.full(n + 2, GUARD, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()      # torch's copies run on torch's stream, the kernels on the context's
    ctx._check(ctx.lib.me_op_exclusive_scan_u32(ctx.handle, C.c_void_p(dc.data_ptr()) if n else None, n, base, form,
                                                C.c_void_p(out.data_ptr())))
    ctx.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert got[n + 1] == GUARD
    return got[:n + 1]


@pytest.mark.parametrize("values", ["random", "zeros", "last"])
@pytest.mark.parametrize("form,n", [(f, n) for f in SIZES for n in SIZES[f]])
def test_offsets_equal_cumsum(form, n, values):
    ctx = _ctx()
    counts, want = _case(n, values)
    if values == "random" and n >= 255:
        assert int(want[n]) > 1 << 32      # a 32-bit accumulator would fail
    for base in BASES:
        got = _scan(ctx, counts, base, form)
        assert np.array_equal(got, want + np.uint64(base)), (form, n, values, base)


def test_form0_of_nothing_is_the_base():
    ctx = _ctx()
    for base in BASES:
        assert _scan(ctx, np.zeros(0, np.uint32), base, 0).tolist() == [base]


def test_host_pointers():
    ctx = _ctx()
    counts, want = _case(1025, "random")
    for form in (0, 1):
        out = np.full(1027, GUARD, np.uint64)
        ctx._check(ctx.lib.me_op_exclusive_scan_u32(ctx.handle, C.c_void_p(counts.ctypes.data), 1025, 7, form,
                                                    C.c_void_p(out.ctypes.data)))
        assert np.array_equal(out[:1026], want + np.uint64(7)) and out[1026] == GUARD


def test_refusals():
    ctx = _ctx()
    counts = np.ones(4, np.uint32)
    out = np.zeros(5, np.uint64)
    cp, op = C.c_void_p(counts.ctypes.data), C.c_void_p(out.ctypes.data)
    for n, form, word in ((-1, 0, b"bad argument"), (-1, 1, b"bad argument"), (0, 1, b"form 1 with 0 counts"),
                          (4, 2, b"form 2"), (4, -1, b"form -1")):
        assert ctx.lib.me_op_exclusive_scan_u32(ctx.handle, cp, n, 0, form, op) == ME_ERR_BAD_ARG, (n, form)
        assert word in ctx.lib.me_last_error(ctx.handle), (n, form)
    assert not out.any()
