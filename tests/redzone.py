"""Red-zone fences for the kernel-level tests.  A plain module: no test lives here.

A Fence is ONE torch.uint8 allocation laid out as [front guard | payload | back guard].  The payload is what a C-ABI entry is
given; the guards are GUARD bytes of a known fill on both sides of it, so that
  * a write outside the operand changes a guard byte and tampered() names its offset, and
  * a read outside the operand reads the fill -- 0xFF, which is NaN in every type the library reads (f16 / bf16 0xFFFF, f32
    0xFFFFFFFF, e4m3fn 0xFF, e8m0 0xFF), or 0x00, which is zero in all of them -- so a result that depends on such a read differs
    between the two fills, or is NaN under the first.
Either access stays inside the allocation: the guard (1 MiB) is larger than anything a kernel in spec may touch beyond an operand
-- the largest single-tile footprint of the cases that use it is a 352-row tile of 256-element 16-bit rows (176 KiB), the next an
18-row halo of a 34-pixel, 256-channel map (about 306 KiB); footprint() asserts a case's own figure against MAX_FOOTPRINT.

The payload starts ALIGN-byte aligned and ends exactly nbytes later: the next byte is already guard (the alignment slack sits in
front of the front guard, never between payload and guard).  Works on CPU tensors as well (tests/test_redzone_cpu.py)."""
import torch

GUARD = 1 << 20
ALIGN = 256
MAX_FOOTPRINT = 512 << 10
FILLS = (0xFF, 0x00)


def footprint(nbytes: int) -> int:
    """A case states the bytes one tile of its kernel may span beyond an operand's start; they must stay well inside a guard."""
    assert 0 <= nbytes < MAX_FOOTPRINT < GUARD, nbytes
    return nbytes


class Fence:
    def __init__(self, nbytes: int, fill: int, device="cuda"):
        assert nbytes >= 0 and 0 <= fill <= 0xFF
        self.nbytes, self.fill = int(nbytes), int(fill)
        self.raw = torch.full((2 * GUARD + self.nbytes + ALIGN,), self.fill, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.raw.data_ptr() + GUARD)) % ALIGN       # offset of the payload in raw
        self.front = self.raw[self.start - GUARD:self.start]
        self.payload = self.raw[self.start:self.start + self.nbytes]
        self.back = self.raw[self.start + self.nbytes:self.start + self.nbytes + GUARD]
        self._snap = None

    def data_ptr(self) -> int:
        return self.raw.data_ptr() + self.start

    def view(self, dtype, shape):
        """The payload as a tensor of `dtype` and `shape` (which must fill it exactly)"""
        n = 1
        for s in shape:
            n *= int(s)
        assert n * torch.empty((), dtype=dtype).element_size() == self.nbytes, (shape, dtype, self.nbytes)
        if self.nbytes == 0:
            return torch.empty(tuple(shape), dtype=dtype, device=self.raw.device)
        return self.payload.view(dtype).view(tuple(shape))

    def tampered(self):
        """Offsets, relative to the payload's start, of the guard bytes that no longer hold the fill: negative in the front guard,
        nbytes .. nbytes + GUARD - 1 in the back guard.  Empty when the fence is clean."""
        f = torch.nonzero(self.front != self.fill).flatten() - GUARD
        b = torch.nonzero(self.back != self.fill).flatten() + self.nbytes
        return [int(x) for x in torch.cat([f, b]).cpu()]

    def snapshot(self):
        self._snap = self.payload.clone()

    def unchanged(self) -> bool:
        assert self._snap is not None
        return bool(torch.equal(self.payload, self._snap))


class FenceSet:
    """The fences of one call under one fill.  inp(): an input operand holding the given values (snapshotted); out(): an output
    whose payload holds the fill; inout(): an operand the entry updates in place.  check() is assertions (c) and (d)."""

    def __init__(self, fill: int, device="cuda"):
        self.fill, self.device = fill, device
        self.inputs, self.outputs = [], []

    def inp(self, values: torch.Tensor):
        if values is None:
            return None
        values = values.contiguous()
        f = Fence(values.numel() * values.element_size(), self.fill, self.device)
        v = f.view(values.dtype, values.shape)
        v.copy_(values)
        f.snapshot()
        self.inputs.append(f)
        return v

    def out(self, dtype, shape):
        n = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            n *= int(s)
        f = Fence(n, self.fill, self.device)
        self.outputs.append(f)
        return f.view(dtype, shape)

    def inout(self, values: torch.Tensor):
        values = values.contiguous()
        f = Fence(values.numel() * values.element_size(), self.fill, self.device)
        v = f.view(values.dtype, values.shape)
        v.copy_(values)
        self.outputs.append(f)
        return v

    def check(self):
        for i, f in enumerate(self.inputs):
            t = f.tampered()
            assert not t, ("input %d: guard bytes written" % i, self.fill, t[:8], len(t))
            assert f.unchanged(), ("input %d: payload changed" % i, self.fill)
        for i, f in enumerate(self.outputs):
            t = f.tampered()
            assert not t, ("output %d: guard bytes written" % i, self.fill, t[:8], len(t))


def is_fill(t: torch.Tensor, fill: int) -> torch.Tensor:
    """Per element: do all its bytes still hold the fill?"""
    size = t.element_size()
    b = t.contiguous().view(torch.uint8).reshape(-1, size)
    return (b == fill).all(dim=1).reshape(t.shape)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))
