"""Cases and the reference of the weight-packer tests (test_weight_pack_cpu.py, test_gpu_weight_pack.py): a numpy / torch
restatement of the four arena layouts and the two conversions that shares nothing with csrc/weight_pack.h.  Layouts:
util.pack_conv / util.pack_convt and a concatenation along the last axis for `dup`; conversions: numpy's astype(float16)
(round to nearest even) and the integer bf16 rule; an f64 source goes through astype(float32) first."""
import numpy as np
import torch

import util

K_VEC_F32, K_MAT_16, K_CONV_16, K_CONVT_16, K_CONVK_F32 = 0, 1, 2, 3, 4
W_F32, W_F16, W_BF16, W_F64 = 0, 1, 2, 3
SRC_NAMES = {W_F32: "f32", W_F16: "f16", W_BF16: "bf16", W_F64: "f64"}
CTX_DTYPES = {"f16": 0, "bf16": 1}

# (name, kind, dims, dup): nothing is a multiple of a tile (64 input channels, 16 output channels of a ConvTranspose) or of a
# 16-byte store, and Cin / Cout sit on both sides of the tile edges
CASES = []
for cout, cin, k in ((3, 5, 3), (2, 33, 3), (65, 257, 3), (4, 8, 1)):
    for dup in (0, 1):
        CASES.append((f"conv{cout}x{cin}x{k}{'d' if dup else ''}", K_CONV_16, (cout, cin, k, k), dup))
for cin, cout in ((5, 7), (33, 3), (257, 65)):
    for dup in (0, 1):
        CASES.append((f"convt{cin}x{cout}{'d' if dup else ''}", K_CONVT_16, (cin, cout, 2, 2), dup))
for n, kdim in ((3, 5), (7, 257)):
    for dup in (0, 1):
        CASES.append((f"mat{n}x{kdim}{'d' if dup else ''}", K_MAT_16, (n, kdim), dup))
# beyond the list above: Cin a multiple of 8, where the transposing kernels store 16 bytes per lane (one tile and a ragged second one)
for dup in (0, 1):
    CASES.append((f"conv3x72x3{'d' if dup else ''}", K_CONV_16, (3, 72, 3, 3), dup))
    CASES.append((f"convt8x3{'d' if dup else ''}", K_CONVT_16, (8, 3, 2, 2), dup))
    CASES.append((f"convt72x17{'d' if dup else ''}", K_CONVT_16, (72, 17, 2, 2), dup))
CASES.append(("vec1", K_VEC_F32, (1,), 0))
CASES.append(("vec257", K_VEC_F32, (257,), 0))
CASES.append(("convk5x3", K_CONVK_F32, (1, 5, 3, 3), 0))
CASE_IDS = [c[0] for c in CASES]

# the values every conversion must get right (as f64; each source type takes what it can represent of them)
SPECIALS = np.array([
    0.0, -0.0,
    2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14,   # f16 subnormals, ties
    1023.5 * 2.0 ** -24, 5 * 2.0 ** -26,
    65504.0, -65504.0, 65519.9, 65520.0, -65520.0, 65536.0, 1e9,                # the last finite half, the first inf
    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23,     # f16 ties on both sides of even
    1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126,                                  # f32 subnormals
    np.inf, -np.inf, np.nan,
    1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, float(np.array([0x7F7F8000], np.uint32).view(np.float32)[0]),   # bf16 ties; the tie that rounds to inf
    1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -8 + 2.0 ** -30,                   # f64: rounding through f32 lands on the tie, directly above it
    2.0 ** -25 + 2.0 ** -60, 65520.0 - 2.0 ** -20,
], dtype=np.float64)


def source(dims, src_dtype, seed):
    """A tensor of `dims` in the source type: normal values with SPECIALS spread over it.  f16 / bf16 come back as their
    uint16 bit patterns (numpy has no bf16), f32 / f64 as such."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    v = rng.standard_normal(n) * 3.0
    step = max(1, n // len(SPECIALS))
    at = (np.arange(len(SPECIALS)) * step) % n
    v[at] = SPECIALS[: len(at)]
    with np.errstate(over="ignore", invalid="ignore"):
        if src_dtype == W_F64:
            out = v
        elif src_dtype == W_F32:
            out = v.astype(np.float32)
        elif src_dtype == W_F16:
            out = v.astype(np.float16).view(np.uint16)
        else:
            out = (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)   # truncation: any bf16 pattern is a fine source
            out[np.isnan(v)] = 0x7FC1
    return np.ascontiguousarray(out.reshape(dims))


def _as_f32(src, src_dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        if src_dtype == W_F16:
            return src.view(np.float16).astype(np.float32)
        if src_dtype == W_BF16:
            return (src.astype(np.uint32) << 16).view(np.float32)
        return src.astype(np.float32)          # f64 rounds to f32 first: part of the contract


def _to_bf16_bits(f32):
    u = f32.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    out[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return out


def expected(kind, dims, dup, src, src_dtype, ctx_dtype):
    """(bits, nan mask) the arena slot must hold: uint16 for the 16-bit kinds, uint32 for the f32 kinds, flat"""
    f32 = _as_f32(src, src_dtype)
    if kind in (K_VEC_F32, K_CONVK_F32):
        bits = f32.view(np.uint32)
        if kind == K_CONVK_F32:
            bits = np.ascontiguousarray(bits.reshape(dims)[0].transpose(1, 2, 0))      # [Cin][k][k] -> [k][k][Cin]
        bits = bits.reshape(-1)
        return bits, (bits & 0x7FFFFFFF) > 0x7F800000
    if ctx_dtype == "bf16":
        b16 = _to_bf16_bits(f32)
        nan_of = lambda b: (b & 0x7FFF) > 0x7F80                                      # noqa: E731
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            b16 = src.copy() if src_dtype == W_F16 else f32.astype(np.float16).view(np.uint16)
        nan_of = lambda b: (b & 0x7FFF) > 0x7C00                                      # noqa: E731
    t = torch.from_numpy(b16.view(np.int16).reshape(dims))
    if kind == K_CONV_16:
        co, ci, kh, kw = dims
        t = util.pack_conv(t).reshape(co, kh * kw, ci)
    elif kind == K_CONVT_16:
        t = util.pack_convt(t)
    else:
        t = t.reshape(dims[0], -1)
    if dup:
        t = torch.cat([t, t], dim=-1)
    bits = t.contiguous().numpy().view(np.uint16).reshape(-1)
    return bits, nan_of(bits)


def nan_mask(bits, ctx_dtype, kind):
    if kind in (K_VEC_F32, K_CONVK_F32):
        return (bits & 0x7FFFFFFF) > 0x7F800000
    return (bits & 0x7FFF) > (0x7F80 if ctx_dtype == "bf16" else 0x7C00)


def check(got, kind, dims, dup, src, src_dtype, ctx_dtype):
    """asserts that `got` (flat bits) is the reference, NaNs compared as NaN only"""
    want, want_nan = expected(kind, dims, dup, src, src_dtype, ctx_dtype)
    got = np.asarray(got).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(nan_mask(got, ctx_dtype, kind), want_nan), "a NaN must stay a NaN, and nothing else become one"
    bad = np.flatnonzero((got != want) & ~want_nan)
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[:5]}: got {got[bad[:5]]}, want {want[bad[:5]]}"


def dst_dtype(kind):
    return np.uint32 if kind in (K_VEC_F32, K_CONVK_F32) else np.uint16


def dst_elems(kind, dims, dup):
    return int(np.prod(dims)) * (2 if dup and kind in (K_MAT_16, K_CONV_16, K_CONVT_16) else 1)
