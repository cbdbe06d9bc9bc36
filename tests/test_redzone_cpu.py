"""tests/redzone.py on CPU tensors: the fence reports what was done to it, at the right offset, and nothing else."""
import pytest
import torch

import redzone as RZ


@pytest.mark.parametrize("fill", RZ.FILLS)
def test_clean_fence_and_layout(fill):
    f = RZ.Fence(1000, fill, "cpu")
    assert f.tampered() == []
    assert f.data_ptr() % RZ.ALIGN == 0
    assert f.front.numel() == RZ.GUARD and f.back.numel() == RZ.GUARD and f.payload.numel() == 1000
    assert f.front.data_ptr() + RZ.GUARD == f.data_ptr() and f.back.data_ptr() == f.data_ptr() + 1000
    assert f.front.data_ptr() >= f.raw.data_ptr()
    assert f.back.data_ptr() + RZ.GUARD <= f.raw.data_ptr() + f.raw.numel()
    assert bool((f.raw == fill).all())          # an output's payload holds the fill too


@pytest.mark.parametrize("fill", RZ.FILLS)
def test_tampering_is_reported_at_its_offset(fill):
    n = 4096
    other = fill ^ 0x5A
    for where, offset in ((("front", 0), -RZ.GUARD), (("front", RZ.GUARD - 1), -1), (("front", 12345), 12345 - RZ.GUARD),
                          (("back", 0), n), (("back", RZ.GUARD - 1), n + RZ.GUARD - 1)):
        f = RZ.Fence(n, fill, "cpu")
        getattr(f, where[0])[where[1]] = other
        assert f.tampered() == [offset], where
    f = RZ.Fence(n, fill, "cpu")
    f.front[-1] = other
    f.back[0] = other
    f.back[-1] = other
    assert f.tampered() == [-1, n, n + RZ.GUARD - 1]
    # a write into the payload is not the guards' business
    f = RZ.Fence(n, fill, "cpu")
    f.payload[:] = other
    assert f.tampered() == []


def test_payload_round_trips_through_view():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 33, generator=g)
    f = RZ.Fence(x.numel() * 4, 0xFF, "cpu")
    v = f.view(torch.float32, x.shape)
    assert v.data_ptr() == f.data_ptr()
    v.copy_(x)
    assert torch.equal(f.view(torch.float32, (7 * 33,)), x.flatten())
    assert torch.equal(f.payload, x.view(torch.uint8).flatten())
    assert f.tampered() == []
    f.snapshot()
    assert f.unchanged()
    v[3, 5] += 1.0
    assert not f.unchanged()
    with pytest.raises(AssertionError):
        f.view(torch.float32, (7, 32))          # a view must fill the payload exactly


def test_ff_fill_is_nan_in_every_type_and_00_is_zero():
    for dtype, size in ((torch.float16, 2), (torch.bfloat16, 2), (torch.float32, 4), (torch.float8_e4m3fn, 1)):
        v = RZ.Fence(64 * size, 0xFF, "cpu").view(dtype, (64,))
        assert bool(torch.isnan(v.float()).all()), dtype
        assert bool(RZ.is_fill(v, 0xFF).all())
        z = RZ.Fence(64 * size, 0x00, "cpu").view(dtype, (64,))
        assert bool((z.float() == 0).all()), dtype
        # the guards read the same way
        f = RZ.Fence(64 * size, 0xFF, "cpu")
        assert bool(torch.isnan(f.back[:64 * size].view(dtype).float()).all()), dtype
        assert bool(torch.isnan(f.front[-64 * size:].view(dtype).float()).all()), dtype
    # e8m0: 0xFF is the NaN code of the scale type by definition (OCP MX, 2^(e - 127) with e = 255 reserved for NaN)
    assert int(RZ.Fence(4, 0xFF, "cpu").payload[0]) == 0xFF


@pytest.mark.parametrize("nbytes", [0, 1, 3, 255, 257, 4101])
def test_odd_payload_ends_flush_against_the_guard(nbytes):
    f = RZ.Fence(nbytes, 0xFF, "cpu")
    assert f.data_ptr() % RZ.ALIGN == 0
    assert f.back.data_ptr() == f.data_ptr() + nbytes
    f.payload.fill_(0x11)
    assert f.tampered() == []
    f.raw[f.start + nbytes] = 0x11              # the very next byte is guard
    assert f.tampered() == [nbytes]


def test_fence_set_and_fill_helpers():
    fs = RZ.FenceSet(0xFF, "cpu")
    a = fs.inp(torch.arange(12, dtype=torch.float32).reshape(3, 4))
    o = fs.out(torch.float16, (5, 3))
    x = fs.inout(torch.ones(2, 2))
    assert fs.inp(None) is None
    assert bool(RZ.is_fill(o, 0xFF).all()) and not bool(RZ.is_fill(a, 0xFF).any())
    o[1:3] = 2.0
    x += 1.0
    fs.check()
    assert RZ.is_fill(o, 0xFF)[:, 0].tolist() == [True, False, False, True, True]
    a[0, 0] = 5.0
    with pytest.raises(AssertionError):
        fs.check()
    assert RZ.same_bits(o, o.clone()) and not RZ.same_bits(o, torch.zeros_like(o))
    with pytest.raises(AssertionError):
        RZ.footprint(RZ.MAX_FOOTPRINT)
    assert RZ.footprint(176 << 10) == 176 << 10
