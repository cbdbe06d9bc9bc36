"""The row-segmented forms of attention and LayerNorm and the fp8 outputs of the forward pass's attention kernels, at kernel
level (-m gpu; me_op_attention_segments, me_op_layernorm_segments).  The encoder runs its three ViTs as one row space
(csrc/pipeline.hip MergedVit, csrc/common.h RowSegs): attention maps a window to its first row, LayerNorm picks its weights
by the segment a row lies in.  The row map changes addresses, not arithmetic, so the segmented launches are held BIT FOR BIT
to the unsegmented entries on the same windows (which are held to fp64), every row of no window must keep its sentinel,
and the fp8 outputs are held code for code to the MX rule (tests/mx_ref.py) applied to the 16-bit output of the same
kernel.  The row map itself is tests/row_segments_ref.py, checked without a GPU by test_row_segments_cpu.py.

Every buffer carries `tokens` guard rows behind the row space: a window written one window off lands in them (and fails
the sentinel check) instead of outside the allocation."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import row_segments_ref as R
from mx_ref import E4M3, quantize_ref, scale_positions
from util import TORCH16, ctx_for, max_err_over_max, ptr, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
OUT_EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}   # one rounding of a 16-bit output
QSCALE = 0.125 * 1.4426950408889634                # common.h kAttnQScale: 1/sqrt(64) * log2(e)
BAD_ARG, BAD_SHAPE = 1, 2
SENTINEL16, SENTINEL8 = 7.0, 0xA5
PAD_FILL = 300.0       # what the rows of no window hold on the input side: a key read from one would own its softmax

ATT_ENV = ("ME_ATT_V", "ME_ATT_HALVES", "ME_ATT_MINW", "ME_ATT_GRID", "ME_ATT_THR")
# mode -> (prescaled, environment): attention_kernel; attention2_kernel; attention3_kernel; attention2p_kernel;
# attention2_kernel<T, 4, true>.  The launcher reads the environment per call.
MODES = {"plain": (0, {}), "prescaled": (1, {}), "v3": (1, {"ME_ATT_V": "3"}), "v4": (1, {"ME_ATT_V": "4"}),
         "halves": (1, {"ME_ATT_HALVES": "1"})}


def _case_id(case):
    return "T{}-W1_{}-W0_{}-h{}-fov{}".format(*case)


def _set_env(monkeypatch, env):
    for k in ATT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed_qkv(lay, heads, dtype, prescaled, variant):
    """the windows back to back: [windows * tokens][3 * heads * 64] in the 16-bit type, on the host"""
    Cc, rows = heads * 64, lay.windows * lay.tokens
    g = torch.Generator().manual_seed(lay.tokens * 7 + lay.windows * 131 + heads + 1000 * prescaled)
    x = torch.randn(rows, 3 * Cc, generator=g) * 1.5
    if variant == "zero_block":      # V columns 32..63 of head 0: an all-zero MX block in every row of that head
        x[:, 2 * Cc + 32:2 * Cc + 64] = 0.0
    elif variant == "near_max":      # every output column near +-1e4 .. 3e4, the top of f16
        base = (1e4 + 2e4 * torch.rand(Cc, generator=g)) * torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
        x[:, 2 * Cc:] = base * (1 + 0.01 * torch.randn(rows, Cc, generator=g))
    else:
        assert variant == "randn"
    if prescaled:
        x[:, :Cc] *= QSCALE
    return x.to(TORCH16[dtype])


@functools.lru_cache(maxsize=None)
def _reference(lay, heads, dtype, prescaled, variant):
    """fp64 softmax attention of the packed windows (computed once per input)"""
    W, T = lay.windows, lay.tokens
    xx = _packed_qkv(lay, heads, dtype, prescaled, variant).cuda().double().reshape(W, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (xx[0] @ xx[1].transpose(3, 2)) * (math.log(2.0) if prescaled else 0.125)     # exp2(s) = exp(s ln 2)
    return (torch.softmax(s, dim=3) @ xx[2]).transpose(1, 2).reshape(W * T, heads * 64).cpu()


def _window_index(lay):
    """row of the row space for every row of the packed windows, in packed order"""
    return torch.tensor([r0 + t for r0 in R.window_rows(lay) for t in range(lay.tokens)], dtype=torch.int64)


def _scatter(packed, lay):
    """packed windows -> the row space (+ guard rows), rows of no window = PAD_FILL"""
    out = torch.full((lay.rows_total + lay.tokens, packed.shape[1]), PAD_FILL, dtype=packed.dtype)
    out[_window_index(lay)] = packed
    return out


def _no_window(lay):
    mask = torch.ones(lay.rows_total + lay.tokens, dtype=torch.bool)
    mask[_window_index(lay)] = False
    return mask


def _segments_call(ctx, lay, heads, prescaled, qkv, out16, out8, out8_scale, **override):
    a = dict(windows=lay.windows, tokens=lay.tokens, heads=heads, prescaled=prescaled, rows_total=lay.rows_total,
             seg1=lay.seg1, seg2=lay.seg2, win0=lay.win0, win1=lay.win1)
    a.update(override)
    return ctx.lib.me_op_attention_segments(ctx.handle, ptr(qkv), ptr(out16), ptr(out8), ptr(out8_scale), a["windows"],
                                            a["tokens"], a["heads"], a["prescaled"], a["rows_total"], a["seg1"], a["seg2"],
                                            a["win0"], a["win1"])


def _run_segmented16(ctx, lay, heads, dtype, prescaled, qkv_dev):
    out = torch.full((lay.rows_total + lay.tokens, heads * 64), SENTINEL16, dtype=TORCH16[dtype], device="cuda")
    torch.cuda.synchronize()
    ctx._check(_segments_call(ctx, lay, heads, prescaled, qkv_dev, out, None, None))
    ctx.synchronize()
    return out.cpu()


def _run_packed16(ctx, lay, heads, dtype, prescaled, packed_dev):
    rows = lay.windows * lay.tokens
    out = torch.full((rows + 1, heads * 64), SENTINEL16, dtype=TORCH16[dtype], device="cuda")
    torch.cuda.synchronize()
    fn = ctx.lib.me_op_attention_prescaled if prescaled else ctx.lib.me_op_attention
    ctx._check(fn(ctx.handle, ptr(packed_dev), ptr(out), lay.windows, lay.tokens, heads))
    ctx.synchronize()
    out = out.cpu()
    assert bool((out[rows] == SENTINEL16).all())
    return out[:rows]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_over_row_segments(dtype, case, mode, monkeypatch):
    """Every attention kernel over a segmented row space: each window's rows are bit for bit what the unsegmented entry
    writes for the same windows packed back to back (same kernel, same environment), which meets the attention bounds
    against fp64; every row of no window (the segments' padding and the guard) still holds the sentinel."""
    tokens, W1, W0, heads, fov = case
    lay = R.layout(tokens, W1, W0, fov)
    prescaled, env = MODES[mode]
    _set_env(monkeypatch, env)
    ctx = ctx_for("tiny", dtype)
    packed = _packed_qkv(lay, heads, dtype, prescaled, "randn")
    got = _run_segmented16(ctx, lay, heads, dtype, prescaled, _scatter(packed, lay).cuda())
    want = _run_packed16(ctx, lay, heads, dtype, prescaled, packed.cuda())
    stray = (got[_no_window(lay)] != SENTINEL16).any(dim=1).nonzero().flatten()
    assert stray.numel() == 0, ("rows of no window were written", _no_window(lay).nonzero().flatten()[stray][:8].tolist())
    g = got[_window_index(lay)]
    for w in range(lay.windows):
        rows = slice(w * tokens, (w + 1) * tokens)
        assert torch.equal(g[rows], want[rows]), ("window", w, "first row", R.window_rows(lay)[w])
    ref = _reference(lay, heads, dtype, prescaled, "randn")
    assert bool(torch.isfinite(want.float()).all())
    assert max_err_over_max(want.float(), ref) < 2 * OUT_EPS[dtype]
    assert rel_l2(want.float(), ref) < 1.5 * OUT_EPS[dtype]


def _fp8_output_check(ctx, lay, heads, mode, variant, monkeypatch):
    """The fp8 epilogue of the kernel `mode` selects: bytes and scale bytes of every window row are the MX rule applied to
    the 16-bit output of the same kernel over the same row space; nothing else is written."""
    prescaled, env = MODES[mode]
    _set_env(monkeypatch, env)
    T, Cc, rows_total = lay.tokens, heads * 64, lay.rows_total
    qkv = _scatter(_packed_qkv(lay, heads, "f16", prescaled, variant), lay).cuda()
    out16 = _run_segmented16(ctx, lay, heads, "f16", prescaled, qkv)
    mt = (rows_total + 127) // 128
    o8 = torch.full((rows_total + T, Cc), SENTINEL8, dtype=torch.uint8, device="cuda")
    # mt tiles of scales for each of the Cc / 128 column groups, and room for the guard rows' tiles behind the last group
    osc = torch.full(((Cc // 128 * mt + (T + 127) // 128 + 2) * 512,), SENTINEL8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx._check(_segments_call(ctx, lay, heads, prescaled, qkv, None, o8, osc))
    ctx.synchronize()
    idx = _window_index(lay)
    want16 = out16[idx].float()
    assert bool(torch.isfinite(want16).all())
    q_ref, sb_ref = quantize_ref(want16)
    got8 = o8.cpu()
    assert bool((got8[_no_window(lay)] == SENTINEL8).all()), "bytes of rows of no window were written"
    bad = (got8[idx].view(E4M3).float() != q_ref.float()).nonzero()       # e4m3 codes compared as values: +0 == -0
    assert bad.numel() == 0, (bad[:8].tolist(), int(bad.shape[0]))
    pos = scale_positions(ctx, rows_total, Cc, 0, idx.tolist())
    host = osc.cpu().numpy()
    assert len(np.unique(pos)) == pos.size and pos.max() < mt * 128 * Cc // 32
    bad = np.argwhere(host[pos] != sb_ref.numpy())
    assert bad.size == 0, (bad[:8].tolist(), len(bad))
    untouched = np.ones(host.size, bool)
    untouched[pos.ravel()] = False
    assert bool((host[untouched] == SENTINEL8).all()), "scale bytes of rows of no window were written"
    if variant == "zero_block":
        assert bool((want16[:, 32:64] == 0).all()) and bool((sb_ref[:, 1] == 0).all())
        assert bool((got8[idx][:, 32:64].view(E4M3).float() == 0).all())
    if variant == "near_max":
        assert 2.5e4 < float(want16.abs().max()) < 6.5e4 and float(want16.abs().min()) > 5e3


FP8_CASES = [(c, "randn") for c in R.CASES] + [(R.CASES[0], "zero_block"), (R.CASES[2], "near_max")]


@pytest.mark.parametrize("mode", ["prescaled", "v3", "v4"])
@pytest.mark.parametrize("case,variant", FP8_CASES, ids=[_case_id(c) + "-" + v for c, v in FP8_CASES])
def test_attention_fp8_output_over_row_segments(case, variant, mode, monkeypatch):
    """attention2_kernel (what an fp8 context's forward pass runs: pre-scaled Q, segments, out8), attention3_kernel and
    attention2p_kernel"""
    tokens, W1, W0, heads, fov = case
    _fp8_output_check(ctx_for("tiny", "f16"), R.layout(tokens, W1, W0, fov), heads, mode, variant, monkeypatch)


def test_attention_fp8_output_over_row_segments_plain_q(monkeypatch):
    """attention_kernel (a plain Q) over segments"""
    tokens, W1, W0, heads, fov = R.CASES[0]
    _fp8_output_check(ctx_for("tiny", "f16"), R.layout(tokens, W1, W0, fov), heads, "plain", "randn", monkeypatch)


@pytest.mark.parametrize("mode", ["prescaled", "v3", "v4"])
@pytest.mark.parametrize("windows,tokens,heads", [(3, 577, 4), (5, 65, 2), (2, 130, 16)])
def test_attention_fp8_output_unsegmented(windows, tokens, heads, mode, monkeypatch):
    """the same kernels without segments (seg1 = 0), at the shapes of test_attention_fp8_output_equals_quantised_16bit_output:
    me_op_attention_fp8 reaches only attention_kernel"""
    _fp8_output_check(ctx_for("tiny", "f16"), R.unsegmented(tokens, windows), heads, mode, "randn", monkeypatch)


def test_attention_halves_form(monkeypatch):
    """ME_ATT_HALVES=1 (attention2_kernel<T, 4, true>: four waves per SIMD, the row sums on the vector pipe) is compiled and
    selectable, so it is tested: the token counts of test_attention_prescaled_token_counts with a guard row, against fp64.
    Not compared with the default form bit for bit: their row sums round differently (attention.hip, at the launch)."""
    _set_env(monkeypatch, {"ME_ATT_HALVES": "1"})
    ctx = ctx_for("tiny", "f16")
    for tokens in [1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 97, 129, 191, 192, 193, 194, 225, 257, 385, 576, 577, 578, 609, 641]:
        windows, heads = (3, 2) if tokens < 400 else (2, 1)
        lay = R.unsegmented(tokens, windows)
        out = _run_packed16(ctx, lay, heads, "f16", 1, _packed_qkv(lay, heads, "f16", 1, "randn").cuda()).float()
        ref = _reference(lay, heads, "f16", 1, "randn")
        assert max_err_over_max(out, ref) < 2 * OUT_EPS["f16"], tokens
        assert rel_l2(out, ref) < 1.5 * OUT_EPS["f16"], tokens
        last = out.reshape(windows, tokens, heads * 64)[:, -1]          # the last query of every window on its own
        assert rel_l2(last, ref.reshape(windows, tokens, heads * 64)[:, -1]) < 2 * OUT_EPS["f16"], tokens


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_halves_form_running_max_branches(dtype, monkeypatch):
    """the planted input of test_attention_running_max_branches (a dominating key in every 64-key tile, a query with only
    strongly negative scores, a query whose maximum is the single tail key) through the ME_ATT_HALVES=1 form"""
    _set_env(monkeypatch, {"ME_ATT_HALVES": "1"})
    ctx = ctx_for("tiny", dtype)
    tokens, heads, Cc = 577, 1, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randn(tokens, 3 * Cc, generator=g)
    qi = 40
    for t in range(9):                                   # key 64 t + 5 scores (t + 2) * 8 against query 40
        x[64 * t + 5, Cc:2 * Cc] = x[qi, 0:Cc] * (t + 2) * 64.0 / float(x[qi, 0:Cc].pow(2).sum())
    x[576, Cc:2 * Cc] = x[200, 0:Cc] * 5.0               # query 200 attends to the tail key
    u = torch.full((Cc,), 0.125)
    x[:, Cc:2 * Cc] += 4.0 * u
    x[100, 0:Cc] = -175.0 * u                            # query 100 scores every key at -87 +- 22 (natural units)
    xin = x.to(TORCH16[dtype])
    xin[:, :Cc] = (xin[:, :Cc].float() * QSCALE).to(xin.dtype)
    out = _run_packed16(ctx, R.unsegmented(tokens, 1), heads, dtype, 1, xin.cuda())
    xx = xin.double()
    v = xx[:, 2 * Cc:]
    ref = torch.softmax(xx[:, :Cc] @ xx[:, Cc:2 * Cc].T * math.log(2.0), dim=1) @ v
    assert bool(torch.isfinite(out.float()).all())
    assert max_err_over_max(out.float(), ref) < 2 * OUT_EPS[dtype]
    assert float((out[qi].double() - v[64 * 8 + 5]).abs().max()) < 0.03     # the last planted key wins
    assert float((out[200].double() - v[576]).abs().max()) < 0.03


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
LN_LAYOUTS = [(2 * 256 + 300, 256, 512), (2 * 256 + 300, 256, 0), (200, 65, 131)]      # (rows, seg1, seg2); the last: boundaries
LN_DIMS = [256, 1024]                                                                   # inside a workgroup's four rows


def _ln_segments(rows, seg1, seg2):
    return [(0, seg1), (seg1, seg2), (seg2, rows)] if seg2 else [(0, seg1), (seg1, rows)]


@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, dim, seg1, seg2):
    """x with one all-zero row per segment (what padding rows hold) and three weight sets far apart -- w near 1, 2, -1.5 and
    biases near 0, 3, -2: a row on the wrong set is wrong by more than any rounding"""
    g = torch.Generator().manual_seed(rows + dim + seg1 + 3 * seg2)
    x = torch.randn(rows, dim, generator=g) * 3 + 0.5
    zero_rows = [lo + 3 for lo, _ in _ln_segments(rows, seg1, seg2)] + [rows - 2]
    x[zero_rows] = 0.0
    ws = [(wm + 0.02 * torch.randn(dim, generator=g)).cuda() for wm in (1.0, 2.0, -1.5)]
    bs = [(bm + 0.02 * torch.randn(dim, generator=g)).cuda() for bm in (0.0, 3.0, -2.0)]
    return x.cuda(), ws, bs, zero_rows


def _three(tensors, n):
    """the `n` first as a const void* [3], the rest null"""
    return (C.c_void_p * 3)(*[t.data_ptr() if i < n else None for i, t in enumerate(tensors)])


def _boundary_rows(rows, seg1, seg2):
    return sorted({0, seg1 - 1, seg1, rows - 1} | ({seg2 - 1, seg2} if seg2 else set()))


def _segment_of(r, seg1, seg2):
    return 0 if r < seg1 else (1 if (not seg2 or r < seg2) else 2)


@pytest.mark.parametrize("rows,seg1,seg2", LN_LAYOUTS)
@pytest.mark.parametrize("dim", LN_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_over_row_segments(dtype, dim, rows, seg1, seg2):
    """layernorm_kernel with per-row weight sets: every segment's rows are bit for bit me_op_layernorm on that segment
    alone with its weights, asserted per row; an all-zero row gives its segment's bias exactly."""
    ctx = ctx_for("tiny", dtype)
    x, ws, bs, zero_rows = _ln_inputs(rows, dim, seg1, seg2)
    segs = _ln_segments(rows, seg1, seg2)
    y16 = torch.full((rows + 1, dim), SENTINEL16, dtype=TORCH16[dtype], device="cuda")
    y32 = torch.full((rows + 1, dim), SENTINEL16, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx._check(ctx.lib.me_op_layernorm_segments(ctx.handle, ptr(x), _three(ws, len(segs)), _three(bs, len(segs)), seg1, seg2,
                                                ptr(y16), ptr(y32), None, None, rows, dim, LN_EPS))
    want16, want32 = torch.empty_like(y16), torch.empty_like(y32)
    for i, (lo, hi) in enumerate(segs):
        ctx._check(ctx.lib.me_op_layernorm(ctx.handle, ptr(x[lo:hi]), ptr(ws[i]), ptr(bs[i]), ptr(want16[lo:hi]), ptr(want32[lo:hi]),
                                           hi - lo, dim, LN_EPS))
    ctx.synchronize()
    assert bool((y16[rows] == SENTINEL16).all()) and bool((y32[rows] == SENTINEL16).all())
    assert bool(torch.isfinite(y32[:rows]).all()) and bool(torch.isfinite(y16[:rows].float()).all())
    for got, want in ((y16, want16), (y32, want32)):
        bad = (got[:rows] != want[:rows]).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, ("rows on other weights or other arithmetic", bad[:8].tolist(), int(bad.numel()))
        for r in _boundary_rows(rows, seg1, seg2):
            assert torch.equal(got[r], want[r]), ("row", r, "segment", _segment_of(r, seg1, seg2))
    for r in zero_rows:
        b = bs[_segment_of(r, seg1, seg2)]
        assert torch.equal(y32[r], b), r
        assert torch.equal(y16[r], b.to(TORCH16[dtype])), r


@pytest.mark.parametrize("rows,seg1,seg2", LN_LAYOUTS)
@pytest.mark.parametrize("dim", LN_DIMS)
def test_layernorm_fp8_over_row_segments(dim, rows, seg1, seg2):
    """layernorm_fp8_kernel with per-row weight sets: bytes and scale bytes of every segment's rows are me_op_layernorm_fp8's
    on that segment alone (each launch's scales read through me_op_scale_index with its own row count); an all-zero row
    gives the MX form of its segment's bias."""
    ctx = ctx_for("tiny", "f16")
    x, ws, bs, zero_rows = _ln_inputs(rows, dim, seg1, seg2)
    segs = _ln_segments(rows, seg1, seg2)
    nsc = lambda n: (n + 127) // 128 * 128 * dim // 32
    y8 = torch.full((rows + 1, dim), SENTINEL8, dtype=torch.uint8, device="cuda")
    ys = torch.full((nsc(rows),), SENTINEL8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx._check(ctx.lib.me_op_layernorm_segments(ctx.handle, ptr(x), _three(ws, len(segs)), _three(bs, len(segs)), seg1, seg2,
                                                None, None, ptr(y8), ptr(ys), rows, dim, LN_EPS))
    want8 = torch.empty(rows, dim, dtype=torch.uint8, device="cuda")
    want_s = []
    for i, (lo, hi) in enumerate(segs):
        s = torch.zeros(nsc(hi - lo), dtype=torch.uint8, device="cuda")
        ctx._check(ctx.lib.me_op_layernorm_fp8(ctx.handle, ptr(x[lo:hi]), ptr(ws[i]), ptr(bs[i]), ptr(want8[lo:hi]), ptr(s), hi - lo, dim,
                                               LN_EPS))
        want_s.append(s)
    ctx.synchronize()
    assert bool((y8[rows] == SENTINEL8).all())
    pos = scale_positions(ctx, rows, dim, 0)
    host = ys.cpu().numpy()
    got_s = host[pos]
    untouched = np.ones(host.size, bool)
    untouched[pos.ravel()] = False
    assert bool((host[untouched] == SENTINEL8).all())                    # the positions of the rows behind `rows` in the last tile
    ref_s = np.concatenate([s.cpu().numpy()[scale_positions(ctx, hi - lo, dim, 0)] for s, (lo, hi) in zip(want_s, segs)])
    bad = (y8[:rows] != want8).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, ("rows on other weights or other arithmetic", bad[:8].tolist(), int(bad.numel()))
    bad = np.argwhere((got_s != ref_s).any(axis=1)).flatten()
    assert bad.size == 0, ("scale bytes", bad[:8].tolist(), len(bad))
    y8h, want8h = y8.cpu(), want8.cpu()
    for r in _boundary_rows(rows, seg1, seg2):
        assert torch.equal(y8h[r], want8h[r]) and np.array_equal(got_s[r], ref_s[r]), ("row", r, "segment", _segment_of(r, seg1, seg2))
    for r in zero_rows:
        q_ref, sb_ref = quantize_ref(bs[_segment_of(r, seg1, seg2)].cpu()[None])
        assert torch.equal(y8h[r].view(E4M3).float(), q_ref[0].float()), r
        assert np.array_equal(got_s[r], sb_ref[0].numpy()), r


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_row_segment_entries_refuse_bad_arguments():
    """A layout that does not fit would make the kernels read and write outside the buffers: each bad argument returns its
    code before any launch, leaves me_last_error set and the sentinel-filled outputs as they were; a correct call
    afterwards still passes."""
    ctx = ctx_for("tiny", "f16")
    lib, h = ctx.lib, ctx.handle
    tokens, W1, W0, heads, fov = R.CASES[0]
    lay = R.layout(tokens, W1, W0, fov)                   # 65 tokens: segments at 256 / 512 of 768 rows, windows 1 | 1 | 3
    two = R.layout(tokens, W1, W0, 0)                     # segments at 256 of 512 rows, windows 1 | 3
    assert (lay.seg1, lay.seg2, lay.rows_total, lay.win0, lay.win1, lay.windows) == (256, 512, 768, 1, 1, 5)
    Cc = heads * 64
    packed = _packed_qkv(lay, heads, "f16", 1, "randn")
    qkv = _scatter(packed, lay).cuda()
    out16 = torch.full((lay.rows_total + tokens, Cc), SENTINEL16, dtype=torch.float16, device="cuda")
    out8 = torch.full((lay.rows_total + tokens, Cc), SENTINEL8, dtype=torch.uint8, device="cuda")
    osc = torch.full((lay.rows_total * Cc // 32 + 2048,), SENTINEL8, dtype=torch.uint8, device="cuda")
    att = lambda l=lay, o16=out16, o8=None, os_=None, q=qkv, **kw: _segments_call(ctx, l, kw.pop("heads", heads), 1, q, o16, o8, os_, **kw)
    x = torch.randn(200, 256).cuda()
    w, b = torch.ones(256, device="cuda"), torch.zeros(256, device="cuda")
    y16 = torch.full((200, 256), SENTINEL16, dtype=torch.float16, device="cuda")
    y32 = torch.full((200, 256), SENTINEL16, dtype=torch.float32, device="cuda")
    y8 = torch.full((200, 256), SENTINEL8, dtype=torch.uint8, device="cuda")
    ysc = torch.full((256 * 256 // 32,), SENTINEL8, dtype=torch.uint8, device="cuda")
    all3, zero3, first = _three([w, w, w], 3), _three([b, b, b], 3), _three([w, w, w], 1)

    def ln(x_=x, ws=all3, bs=zero3, s1=65, s2=131, o16=y16, o32=None, o8=None, os_=None, rows=200, dim=256):
        return lib.me_op_layernorm_segments(h, ptr(x_), ws, bs, s1, s2, ptr(o16), ptr(o32), ptr(o8), ptr(os_), rows, dim, LN_EPS)

    torch.cuda.synchronize()
    cases = [
        (BAD_ARG, lambda: att(q=None)),                                       # null pointers
        (BAD_ARG, lambda: att(o16=None)),                                     # neither output
        (BAD_ARG, lambda: att(o8=out8, os_=osc)),                             # both
        (BAD_ARG, lambda: att(o16=None, o8=out8)),                            # out8 without its scales
        (BAD_ARG, lambda: att(o16=None, o8=out8, os_=osc, heads=3)),          # an odd head count with out8
        (BAD_ARG, lambda: att(seg2=256)),                                     # segment starts out of order
        (BAD_ARG, lambda: att(seg2=128)),
        (BAD_ARG, lambda: att(seg1=0)),                                       # a third segment without a second
        (BAD_ARG, lambda: att(seg1=1024, seg2=0)),                            # beyond the row space
        (BAD_ARG, lambda: att(win0=-1)),
        (BAD_SHAPE, lambda: att(win0=4, windows=8)),                          # 4 * 65 > seg1 = 256
        (BAD_SHAPE, lambda: att(win1=4, windows=8)),                          # the middle segment's windows reach past seg2
        (BAD_SHAPE, lambda: att(windows=9)),                                  # the last segment's 7 windows past rows_total
        (BAD_SHAPE, lambda: att(windows=1)),                                  # fewer windows than win0 + win1
        (BAD_SHAPE, lambda: att(l=two, win1=4, windows=5)),                   # two segments: the last one's 4 * 65 > 256 rows
        (BAD_SHAPE, lambda: att(l=two, windows=5)),                           # two segments: windows != win0 + win1
        (BAD_SHAPE, lambda: att(seg1=0, seg2=0, windows=12)),                 # no segments: 12 * 65 > 768 rows
        (BAD_SHAPE, lambda: att(tokens=0)),
        (BAD_ARG, lambda: ln(x_=None)),                                       # null pointers
        (BAD_ARG, lambda: ln(ws=first)),                                      # a segment without weights
        (BAD_ARG, lambda: ln(s2=0, bs=first)),
        (BAD_ARG, lambda: ln(o16=None)),                                      # neither output form
        (BAD_ARG, lambda: ln(o8=y8, os_=ysc)),                                # both
        (BAD_ARG, lambda: ln(o16=None, o32=y32, o8=y8, os_=ysc)),
        (BAD_ARG, lambda: ln(o16=None, o8=y8)),                               # y8 without its scales
        (BAD_ARG, lambda: ln(s2=65)),                                         # segment starts out of order
        (BAD_ARG, lambda: ln(s1=0)),
        (BAD_ARG, lambda: ln(s1=300, s2=0)),                                  # beyond `rows`
        (BAD_SHAPE, lambda: ln(dim=100)),
        (BAD_SHAPE, lambda: ln(o16=None, o8=y8, os_=ysc, dim=128)),           # the fp8 form starts at 256
        (BAD_SHAPE, lambda: ln(rows=0, s1=0, s2=0)),
    ]
    for i, (code, call) in enumerate(cases):
        rc = call()
        msg = lib.me_last_error(h)
        assert rc == code, f"case {i}: returned {rc}, expected {code}: {msg}"
        assert msg and (b"me_op_attention_segments" in msg if i < 18 else b"me_op_layernorm_segments" in msg), (i, msg)
    assert lib.me_op_attention_segments(None, ptr(qkv), ptr(out16), None, None, 5, 65, 2, 1, 768, 256, 512, 1, 1) == BAD_ARG
    assert lib.me_op_layernorm_segments(None, ptr(x), all3, zero3, 65, 131, ptr(y16), None, None, None, 200, 256, LN_EPS) == BAD_ARG
    ctx.synchronize()
    for t, s in ((out16, SENTINEL16), (out8, SENTINEL8), (osc, SENTINEL8), (y16, SENTINEL16), (y32, SENTINEL16), (y8, SENTINEL8),
                 (ysc, SENTINEL8)):
        assert bool((t == s).all())                                           # nothing was launched
    # the context works afterwards
    ctx._check(att())
    ctx._check(ln(o32=y32))
    ctx.synchronize()
    want = _run_packed16(ctx, lay, heads, "f16", 1, packed.cuda())
    assert torch.equal(out16.cpu()[_window_index(lay)], want)
    ref = torch.nn.functional.layer_norm(x[:65].double(), (256,))
    assert float((y32[:65].double() - ref).abs().max()) < 2e-5
