"""Stream order (-m gpu): the library on a CALLER's stream (me_ctx_set_stream), the side branch of extract_depth, the
first launch on a stream nobody has seen, and two contexts queuing at once.

Every asynchronous case has the same shape (stream_order.py): a producer keeps the caller's stream busy and writes the
real input LAST, over a poison fill; the library call is queued while the producer is still running (asserted: a case
where it was not did not test ordering and fails); a copy of the result is queued on the caller's stream right behind
the call, and the host waits for that stream only.  Expected values are the library's own: the same calls on the
context's own stream with torch.cuda.synchronize() and ctx.synchronize() around every call, which the rest of the suite
holds to fp64 or the oracle.  Equality is bit for bit, so there is no tolerance to choose."""
import contextlib
import ctypes as C
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
import stream_order as SO
from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
from util import TORCH16, bordered, ctx_for, dev16, loaded_ctx, pack_conv, pack_convt, ptr, weights_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QSCALE = 0.125 * math.log2(math.e)
_OWN = {}


def _grid8_cfg():
    return m.ModelConfig(**SO.GRID8)


def _step_ctx(dtype, cfg_name):
    if cfg_name == "tiny":
        return loaded_ctx("tiny", dtype)
    key = (cfg_name, dtype)
    if key not in _OWN:
        cfg = _grid8_cfg()
        ctx = m.Context(0, dtype, cfg)
        ctx.load_state_dict(synthetic_checkpoint(cfg))
        _OWN[key] = ctx
    return _OWN[key]


@pytest.fixture(scope="module", autouse=True)
def _release_at_the_end():
    """the contexts of this module and the producer's tensors go when its last test has run"""
    yield
    for ctx in _OWN.values():
        ctx.close()
    _OWN.clear()
    SO.release()


@contextlib.contextmanager
def _on_stream(ctx, stream):
    ctx.set_stream(stream.cuda_stream)
    try:
        yield
    finally:
        ctx.set_stream(None)


def _images(S, batch, entry, seed=2024):
    u8 = torch.from_numpy(synthetic_images(batch, S, "structured", seed=seed)).cuda()
    if entry == "u8":
        return u8
    return ((u8.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()


def _call_step(ctx, entry, img, batch, f_norm, out, fov):
    fn = ctx.lib.me_extract_depth_u8 if entry == "u8" else ctx.lib.me_extract_depth
    ctx._check(fn(ctx.handle, ptr(img), batch, ptr(f_norm), ptr(out), ptr(fov)))


def _synced(ctx, call):
    """the reference form: the whole device and the context drained on both sides of the call"""
    torch.cuda.synchronize()
    ctx.synchronize()
    call()
    ctx.synchronize()
    torch.cuda.synchronize()


def _fill7(tensors, stream):
    with torch.cuda.stream(stream):
        for t in tensors:
            if t is not None:
                t.fill_(7)


PICTURES = 3


class _Step:
    """The operands of one me_extract_depth[_u8] case: PICTURES different inputs (each with its own f_norm) that pass through
    the SAME buffers, and the synchronised reference result of each.  The context's workspaces persist from call to call, so
    a case that repeated one picture would find every internal buffer already holding the expected values, and a mid-step
    launch on the wrong stream, a late join or a launch that fell out of the capture would read and write identical data.
    Here call i runs picture i % PICTURES while the workspaces hold the picture before it, whose results differ."""

    def __init__(self, ctx, batch, entry, form, seed=2024):
        S = ctx.cfg.img_size
        self.ctx, self.batch, self.entry = ctx, batch, entry
        pics = _images(S, PICTURES * batch, entry, seed)
        self.reals = [pics[i * batch:(i + 1) * batch].contiguous() for i in range(PICTURES)]
        self.inp = torch.empty_like(self.reals[0])
        base = torch.tensor([0.8, 1.3][:batch], device="cuda")
        self.fn_reals = [base * (1.0 + 0.25 * i) for i in range(PICTURES)] if form == "f_norm" else None
        self.fn = torch.empty_like(base) if form == "f_norm" else None
        self.out = torch.empty(batch, S, S, device="cuda")
        self.fov = torch.empty(batch, device="cuda") if form == "fov" else None
        self.refs = [self.reference(i) for i in range(PICTURES)]
        for i in range(PICTURES):
            for j in range(i):          # stale data of another picture cannot pass for this one's
                assert not torch.equal(self.refs[i][0], self.refs[j][0])
                assert self.fov is None or not torch.equal(self.refs[i][1], self.refs[j][1])

    def writes(self, i):
        return [(self.inp, self.reals[i])] + ([(self.fn, self.fn_reals[i])] if self.fn is not None else [])

    def call(self, out=None):
        _call_step(self.ctx, self.entry, self.inp, self.batch, self.fn, self.out if out is None else out, self.fov)

    def reference(self, i):
        for dst, src in self.writes(i):
            dst.copy_(src)
        _fill7([self.out, self.fov], torch.cuda.current_stream())
        _synced(self.ctx, self.call)
        assert bool(torch.isfinite(self.out).all()) and not bool((self.out == 7.0).all())
        return self.out.clone(), (self.fov.clone() if self.fov is not None else None)

    def queued(self, stream, busy_ms, i, out=None):
        """prefill, producer (writes picture i), library call, consumer on `stream`; returns (i, producer still running,
        depth copy, fov copy)"""
        out = self.out if out is None else out
        _fill7([out, self.fov], stream)
        done = SO.busy(stream, busy_ms, self.writes(i))
        self.call(out)
        running = SO.still_running(done)
        return i, running, SO.snapshot(stream, out), (SO.snapshot(stream, self.fov) if self.fov is not None else None)

    def check(self, results, what):
        for n, (i, running, depth, fov) in enumerate(results):
            assert running, f"{what}, call {n}: the producer had finished before the library call returned -- nothing was ordered"
            assert torch.equal(depth, self.refs[i][0]), f"{what}, call {n}: depth differs from the synchronised reference of picture {i}"
            assert fov is None or torch.equal(fov, self.refs[i][1]), f"{what}, call {n}: fov differs"


# ---- 1. the step on the caller's stream ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cfg_name,batch,entry,form", SO.STEP_CASES)
def test_step_on_the_callers_stream(dtype, cfg_name, batch, entry, form):
    """me_extract_depth / me_extract_depth_u8 with device pointers only, three calls eager and three with the graph on
    (eager, captured, replayed), each between the producer and the consumer on a torch.cuda.Stream() and each on another
    picture than the call before it (the references leave the last picture in the workspaces, the first queued call runs
    the first); then back on the own stream, where the first call is eager again (the graph's key holds the stream)."""
    ctx = _step_ctx(dtype, cfg_name)
    try:
        ctx.set_graph(False)
        step = _Step(ctx, batch, entry, form)
        s = torch.cuda.Stream()
        with _on_stream(ctx, s):
            for graph in (False, True):
                ctx.set_graph(graph)
                n0 = ctx.graph_launch_count
                results = [step.queued(s, SO.busy_ms(), i) for i in range(PICTURES)]
                s.synchronize()                          # the caller's stream only: ctx.synchronize() is not called here
                step.check(results, "graph" if graph else "eager")
                assert ctx.graph_launch_count == n0 + (2 if graph else 0)
            n1 = ctx.graph_launch_count
        # (_on_stream has restored the own stream; the workspaces hold the last picture)
        ref, ref_fov = step.reference(0)
        assert ctx.graph_launch_count == n1, "the first call on another stream must not replay the old stream's graph"
        assert torch.equal(ref, step.refs[0][0]) and (ref_fov is None or torch.equal(ref_fov, step.refs[0][1]))
    finally:
        ctx.set_graph(False)
        ctx.set_stream(None)


@pytest.mark.parametrize("dtype,cfg_name", [("f16", "tiny"), ("fp8", "grid8")])
def test_stream_switch_with_a_replay_in_flight(dtype, cfg_name):
    """A replay queued on one caller stream behind a running producer, then me_ctx_set_stream to a second one and a call
    there: the in-flight result is intact (the switch waits for the stream it leaves before the graph goes), the call on
    the new stream is eager and ordered behind ITS producer.  Every call runs another picture than the one before it."""
    ctx = _step_ctx(dtype, cfg_name)
    try:
        ctx.set_graph(False)
        step = _Step(ctx, 2, "u8", "fov")
        ctx.set_graph(True)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        other = torch.empty_like(step.out)
        ctx.set_stream(s1.cuda_stream)
        warm = [step.queued(s1, SO.busy_ms(), i) for i in range(2)]       # eager, captured
        n0 = ctx.graph_launch_count
        flying = step.queued(s1, SO.busy_ms(), 2)        # the replay, in flight ...
        assert ctx.graph_launch_count == n0 + 1
        ctx.set_stream(s2.cuda_stream)                   # ... when the stream changes
        moved = step.queued(s2, SO.busy_ms(), 0, out=other)
        assert ctx.graph_launch_count == n0 + 1
        s1.synchronize()
        s2.synchronize()
        step.check(warm + [flying, moved], "switch")
    finally:
        ctx.set_graph(False)
        ctx.set_stream(None)


# ---- 2. kernel entries chained on the caller's stream --------------------------------------------------------------------

def _run_chain(ctx, writes, scratch, results, calls, overlap=False):
    """calls: thunks that return an entry's status.  Reference: every call between full synchronisations on the own stream.
    Then the same calls on a caller's stream with no host wait inside the chain, the inputs written by the producer, every
    buffer the chain writes holding 7 beforehand.  overlap: the output back end on the context's second stream, whose results
    the caller reads after me_ctx_synchronize (the contract of me_ctx_set_output_overlap), not behind the call on its stream."""
    for dst, src in writes:
        dst.copy_(src)
    _fill7(scratch, torch.cuda.current_stream())
    for call in calls:
        _synced(ctx, lambda: ctx._check(call()))
    ref = [t.clone() for t in results]
    for t in scratch:
        assert not bool((t.float() == 7).all()), "an output of the chain was never written"
    s = torch.cuda.Stream()
    try:
        if overlap:
            ctx.set_output_overlap(True)
        with _on_stream(ctx, s):
            _fill7(scratch, s)
            done = SO.busy(s, SO.busy_ms(len(calls)), writes)
            for call in calls:
                ctx._check(call())
            running = SO.still_running(done)
            if overlap:
                ctx.synchronize()
                got = results
            else:
                got = [SO.snapshot(s, t) for t in results]
                s.synchronize()
            assert running, "the producer had finished before the chain was queued -- nothing was ordered"
            for i, (a, b) in enumerate(zip(got, ref)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"result {i} differs from the synchronised reference"
    finally:
        if overlap:
            ctx.set_output_overlap(False)


def _admitted(ctx, make_call, tile_cfg):
    """The entry's call with tile_cfg where its table admits the tile, with the automatic choice (-1) where the library
    refuses it (a refusal is a host check that launches nothing: test_refused_tile_configs_report_and_launch_nothing)"""
    if tile_cfg == -1:
        return make_call(-1)
    torch.cuda.synchronize()
    rc = make_call(tile_cfg)()
    ctx.synchronize()
    assert rc in (0, 1, 2), rc
    return make_call(tile_cfg if rc == 0 else -1)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("tile_cfg", [-1, 10])
def test_vit_block_chain(dtype, tile_cfg):
    """One Block::forward from seven entries: 2 windows x 65 tokens, 2 heads (C = 128), hidden 512"""
    ctx, L = ctx_for("tiny", dtype), ctx_for("tiny", dtype).lib
    h, t16 = ctx.handle, TORCH16[dtype]
    windows, tokens, heads, C, hidden = 2, 65, 2, 128, 512
    M = windows * tokens
    g = torch.Generator().manual_seed(65 + C)
    lin = lambda n, k: (dev16(torch.randn(n, k, generator=g) / math.sqrt(k), dtype), torch.randn(n, generator=g).cuda())
    ln = lambda: ((1.0 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda())
    (w_qkv, b_qkv), (w_proj, b_proj), (w_fc1, b_fc1), (w_fc2, b_fc2) = lin(3 * C, C), lin(C, C), lin(hidden, C), lin(C, hidden)
    (ln1w, ln1b), (ln2w, ln2b) = ln(), ln()
    g1, g2 = (0.05 + 0.15 * torch.rand(C, generator=g)).cuda(), (0.05 + 0.15 * torch.rand(C, generator=g)).cuda()
    x_real = (torch.randn(M, C, generator=g) * 2.0).cuda()
    x = torch.empty_like(x_real)
    xn, xn2 = torch.empty(M, C, dtype=t16, device="cuda"), torch.empty(M, C, dtype=t16, device="cuda")
    qkv, att = torch.empty(M, 3 * C, dtype=t16, device="cuda"), torch.empty(M, C, dtype=t16, device="cuda")
    hid = torch.empty(M, hidden, dtype=t16, device="cuda")
    eps = 1e-5
    calls = [
        lambda: L.me_op_layernorm(h, ptr(x), ptr(ln1w), ptr(ln1b), ptr(xn), None, M, C, eps),
        _admitted(ctx, lambda cfg: lambda: L.me_op_linear_scaled_cols(h, M, 3 * C, C, ptr(xn), ptr(w_qkv), ptr(b_qkv), ptr(qkv), C, QSCALE, cfg),
                  tile_cfg),
        lambda: L.me_op_attention_prescaled(h, ptr(qkv), ptr(att), windows, tokens, heads),
        _admitted(ctx, lambda cfg: lambda: L.me_op_linear_residual(h, M, C, C, ptr(att), ptr(w_proj), ptr(b_proj), ptr(g1), ptr(x), cfg), tile_cfg),
        lambda: L.me_op_layernorm(h, ptr(x), ptr(ln2w), ptr(ln2b), ptr(xn2), None, M, C, eps),
        _admitted(ctx, lambda cfg: lambda: L.me_op_linear(h, M, hidden, C, ptr(xn2), ptr(w_fc1), ptr(b_fc1), ptr(hid), None, 1, cfg), tile_cfg),
        _admitted(ctx, lambda cfg: lambda: L.me_op_linear_residual(h, M, C, hidden, ptr(hid), ptr(w_fc2), ptr(b_fc2), ptr(g2), ptr(x), cfg), tile_cfg),
    ]
    assert ctx.status_flags() in (0, 1)      # (drained: the probes of _admitted ran on uninitialised operands)
    _run_chain(ctx, [(x, x_real)], [xn, qkv, att, xn2, hid], [x, xn, qkv, att, xn2, hid], calls)
    assert ctx.status_flags() == 0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fused_layernorm_chain(dtype):
    """me_op_linear_residual_layernorm at N = 256 and a me_op_linear that reads the normalised rows it leaves"""
    ctx, L = ctx_for("tiny", dtype), ctx_for("tiny", dtype).lib
    h, t16 = ctx.handle, TORCH16[dtype]
    M, N, K, N2 = 353, 256, 128, 512
    g = torch.Generator().manual_seed(M + N + K)
    a_real = dev16(torch.randn(M, K, generator=g), dtype)
    a = torch.empty_like(a_real)
    w, b = dev16(torch.randn(N, K, generator=g) / math.sqrt(K), dtype), torch.randn(N, generator=g).cuda()
    gam = (0.05 + 0.15 * torch.rand(N, generator=g)).cuda()
    lw, lb = (1.0 + 0.1 * torch.randn(N, generator=g)).cuda(), (0.1 * torch.randn(N, generator=g)).cuda()
    w2, b2 = dev16(torch.randn(N2, N, generator=g) / math.sqrt(N), dtype), torch.randn(N2, generator=g).cuda()
    x_real = (torch.randn(M, N, generator=g) * 2.0).cuda()
    x = torch.empty_like(x_real)
    xn = torch.empty(M, N, dtype=t16, device="cuda")
    out = torch.empty(M, N2, dtype=torch.float32, device="cuda")
    one = lambda t: (C.c_void_p * 3)(t.data_ptr(), None, None)
    ws, bs, gs, lws, lbs = one(w), one(b), one(gam), one(lw), one(lb)
    calls = [
        lambda: L.me_op_linear_residual_layernorm(h, M, N, K, ptr(a), 0, 0, ws, bs, gs, lws, lbs, 1e-5, ptr(x), ptr(xn)),
        lambda: L.me_op_linear(h, M, N2, N, ptr(xn), ptr(w2), ptr(b2), None, ptr(out), 0, -1),
    ]
    _run_chain(ctx, [(a, a_real), (x, x_real)], [xn, out], [x, xn, out], calls)
    assert ctx.status_flags() == 0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_conv_chain(dtype):
    """me_op_conv2d (3x3, bordered 16-bit output) -> me_op_conv_transpose2x2 over that bordered map -> me_op_head_final:
    1 x 12 x 16 pixels, 128 channels"""
    ctx, L = ctx_for("tiny", dtype), ctx_for("tiny", dtype).lib
    h, t16 = ctx.handle, TORCH16[dtype]
    H, W, Cc, Cmid = 12, 16, 128, 32
    g = torch.Generator().manual_seed(H * W + Cc)
    in_real = bordered(torch.randn(1, Cc, H, W, generator=g), dtype)
    inp = torch.empty_like(in_real)
    w1 = dev16(pack_conv(torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)), dtype)
    b1 = torch.randn(Cc, generator=g).cuda()
    wt = dev16(pack_convt(torch.randn(Cc, Cc, 2, 2, generator=g) / math.sqrt(Cc)), dtype)
    bt = torch.randn(Cc, generator=g).cuda()
    wh = dev16(pack_conv(torch.randn(Cmid, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)), dtype)
    bh, w2, b2 = (torch.randn(Cmid, generator=g) * 0.3).cuda(), (torch.randn(Cmid, generator=g) / math.sqrt(Cmid)).cuda(), torch.tensor([0.4]).cuda()
    H1, W1 = H + 2, W + 2                        # the ConvTranspose reads the bordered map as a map of its own
    mid = torch.empty(1, H1, W1, Cc, dtype=t16, device="cuda")
    up = torch.empty(1, 2 * H1 + 2, 2 * W1 + 2, Cc, dtype=t16, device="cuda")
    out = torch.empty(2 * H1 * 2 * W1, device="cuda")
    inf = float("inf")
    calls = [
        lambda: L.me_op_conv2d(h, ptr(inp), 1, H, W, Cc, ptr(w1), Cc, 3, 1, ptr(b1), None, None, None, ptr(mid), 1, 2, 0, -1),
        lambda: L.me_op_conv_transpose2x2(h, ptr(mid), 1, H1, W1, Cc, ptr(wt), Cc, ptr(bt), None, ptr(up), 1, -1),
        lambda: L.me_op_head_final(h, ptr(up), 1, 2 * H1, 2 * W1, Cc, ptr(wh), Cmid, ptr(bh), ptr(w2), ptr(b2), None, -inf, inf, ptr(out), -1),
    ]
    _run_chain(ctx, [(inp, in_real)], [mid, up, out], [mid, up, out], calls)


def test_fp8_chain():
    """me_op_layernorm_fp8 -> me_op_linear_fp8 (GELU, fp8 output) -> me_op_linear_fp8 (residual update): M = N = K = 256"""
    ctx, L = ctx_for("tiny", "f16"), ctx_for("tiny", "f16").lib
    h = ctx.handle
    M = N = K = 256
    g = torch.Generator().manual_seed(M + N + K)

    def weight8():
        w16 = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
        w8, ws = torch.empty(N, K, dtype=torch.uint8, device="cuda"), torch.zeros(N * K // 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx._check(L.me_op_quantize_fp8(h, ptr(w16), N, K, 1, ptr(w8), ptr(ws)))
        ctx.synchronize()
        return w8, ws, torch.randn(N, generator=g).cuda()

    (w1, w1s, b1), (w2, w2s, b2) = weight8(), weight8()
    lw, lb = (1.0 + 0.1 * torch.randn(K, generator=g)).cuda(), (0.1 * torch.randn(K, generator=g)).cuda()
    gam = (0.05 + 0.15 * torch.rand(N, generator=g)).cuda()
    x_real = (torch.randn(M, K, generator=g) * 3 + 0.5).cuda()
    x = torch.empty_like(x_real)
    y8, ys = torch.empty(M, K, dtype=torch.uint8, device="cuda"), torch.empty(M * K // 32, dtype=torch.uint8, device="cuda")
    h8, hs = torch.empty(M, N, dtype=torch.uint8, device="cuda"), torch.empty(M * N // 32, dtype=torch.uint8, device="cuda")
    calls = [
        lambda: L.me_op_layernorm_fp8(h, ptr(x), ptr(lw), ptr(lb), ptr(y8), ptr(ys), M, K, 1e-5),
        lambda: L.me_op_linear_fp8(h, M, N, K, ptr(y8), ptr(ys), ptr(w1), ptr(w1s), ptr(b1), None, ptr(h8), ptr(hs), None, None),
        lambda: L.me_op_linear_fp8(h, M, N, N, ptr(h8), ptr(hs), ptr(w2), ptr(w2s), ptr(b2), None, None, None, ptr(gam), ptr(x)),
    ]
    _run_chain(ctx, [(x, x_real)], [y8, ys, h8, hs], [x, y8, ys, h8, hs], calls)


@pytest.mark.parametrize("overlap", [False, True])
def test_output_back_end_chain(overlap):
    """me_depth_clamp_minmax_async -> me_depthmap_rgb_dev_range and me_stereogram_keyed_dev_range on a 64 x 64 map, device
    outputs.  overlap = False: ordered on the caller's stream like any other call.  overlap = True
    (me_ctx_set_output_overlap): the inputs are still read behind the producer on the caller's stream, the results are written
    on the context's second stream and read behind me_ctx_synchronize."""
    ctx, L = ctx_for("tiny", "f16"), ctx_for("tiny", "f16").lib
    h, side = ctx.handle, 64
    g = torch.Generator().manual_seed(64)
    d_real = (0.002 + 12.0 * torch.rand(side, side, generator=g) ** 3).cuda()      # both clamps of DepthMap::new bite
    depth = torch.empty_like(d_real)
    minmax = torch.empty(2, device="cuda")
    rgb = torch.empty(side * side, 3, dtype=torch.uint8, device="cuda")
    stereo = torch.empty(side, side, 3, dtype=torch.uint8, device="cuda")
    key = (C.c_uint8 * 32)(*range(1, 33))
    calls = [
        lambda: L.me_depth_clamp_minmax_async(h, ptr(depth), side * side, ptr(minmax)),
        lambda: L.me_depthmap_rgb_dev_range(h, ptr(depth), side * side, ptr(minmax), ptr(rgb)),
        lambda: L.me_stereogram_keyed_dev_range(h, ptr(depth), side, side, ptr(minmax), side, side, 1.0 / 16.0, key, ptr(stereo)),
    ]
    _run_chain(ctx, [(depth, d_real)], [minmax, rgb, stereo], [depth, minmax, rgb, stereo], calls, overlap=overlap)


# ---- 3. the first launch on a stream nobody has seen ---------------------------------------------------------------------

_FIRST_LAUNCH_CHILD = """
import sys
root, tests = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, tests)
import ctypes as C, math, torch
import matrix_eyes_amd as m
import stream_order as SO
M, N, K = SO.FIRST_LAUNCH_SHAPE
g = torch.Generator().manual_seed(M + N + K)
a = (torch.randn(M, K, generator=g)).half().cuda()
w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
bias = torch.randn(N, generator=g).cuda()
ref = a.float() @ w.float().T + bias
bound = 2e-4 * float(ref.abs().max())                 # test_linear_persistent_rounds' bound
outs = {}
for rnd in range(2):
    for cfg in SO.FIRST_LAUNCH_TILES:
        outs[(rnd, cfg)] = torch.full((M, N), 7.0, device="cuda")
torch.cuda.synchronize()
ctx = m.Context(0, "f16", m.ModelConfig.tiny())      # no weights: the op entries need none
p = lambda t: C.c_void_p(t.data_ptr())
copies = {}
streams = []
for rnd in range(2):
    for cfg in SO.FIRST_LAUNCH_TILES:
        s = torch.cuda.Stream()                           # a stream the library has never seen; the first me_op_* call of the process is on one
        streams.append(s)
        ctx.set_stream(s.cuda_stream)
        ctx._check(ctx.lib.me_op_linear(ctx.handle, M, N, K, p(a), p(w), p(bias), None, p(outs[(rnd, cfg)]), 0, cfg))
        copies[(rnd, cfg)] = SO.snapshot(s, outs[(rnd, cfg)])
for s in streams:
    s.synchronize()
ctx.set_stream(None)
for cfg in SO.FIRST_LAUNCH_TILES:
    err = float((copies[(0, cfg)] - ref).abs().max())
    print("tile", cfg, "max error", err, "bound", bound)
    assert err < bound, (cfg, err, bound)
    assert torch.equal(copies[(0, cfg)], copies[(1, cfg)]), cfg
ctx.close()
print("first launch ok")
"""


def test_first_launch_on_a_fresh_stream_in_a_child_process():
    """ME_GEMM_DYNAMIC_TILES=1: the tile-queue block of a stream is allocated and zeroed (hipMemset on the null stream) at the
    stream's first GEMM launch.  The child's first me_op_* call is a multi-round me_op_linear on a fresh torch.cuda.Stream(),
    each tile id on its own fresh stream, twice; fp32 torch within test_linear_persistent_rounds' bound, and the two rounds bit
    for bit.  (Whatever me_ctx_create itself queues is not a GEMM launch and takes no queue block.)  This observes that the
    memset has landed on six fresh streams; it cannot make the race lose, so it is no proof that it never does."""
    env = dict(os.environ, ME_GEMM_DYNAMIC_TILES="1")
    r = subprocess.run([sys.executable, "-c", _FIRST_LAUNCH_CHILD, ROOT, os.path.dirname(os.path.abspath(__file__))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first launch ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 4. the side branch ---------------------------------------------------------------------------------------------------

_SIDE_BRANCH_CHILD = """
import os, sys
root, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, tests)
import ctypes as C, numpy as np, torch
import matrix_eyes_amd as m
import stream_order as SO
from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
want_branch = os.environ.get("ME_OVERLAP_TAIL") == "1"
p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
ctxs, saved = {}, {}
for name, cfg in (("tiny", m.ModelConfig.tiny()), ("grid8", m.ModelConfig(**SO.GRID8))):
    ctxs[name] = m.Context(0, "f16", cfg)
    ctxs[name].load_state_dict(synthetic_checkpoint(cfg))
PICTURES = 3
base, pictures = {}, {}
for cfg_name, batch, form, graph, where in SO.SIDE_BRANCH_RUNS:
    ctx = ctxs[cfg_name]
    S = ctx.cfg.img_size
    # three pictures (and f_norms) through the same buffers: the workspaces a call finds hold another picture's values
    if S not in pictures:
        pictures[S] = torch.from_numpy(synthetic_images(PICTURES * 2, S, "structured", seed=7)).cuda()
    pics = pictures[S]
    reals = [pics[i * batch:(i + 1) * batch].contiguous() for i in range(PICTURES)]
    fn_reals = [torch.tensor([0.8, 1.3][:batch], device="cuda") * (1.0 + 0.25 * i) for i in range(PICTURES)]
    inp = torch.empty_like(reals[0])
    fn = torch.empty_like(fn_reals[0]) if form == "f_norm" else None
    fov = torch.empty(batch, device="cuda") if form == "fov" else None
    out = torch.empty(batch, S, S, device="cuda")
    torch.cuda.synchronize()
    ctx.set_graph(graph)
    s = torch.cuda.Stream() if where == "caller" else None
    ctx.set_stream(s.cuda_stream if s else None)
    b0, g0 = ctx.side_branch_count, ctx.graph_launch_count
    got = []
    for i in range(PICTURES):
        writes = [(inp, reals[i])] + ([(fn, fn_reals[i])] if fn is not None else [])
        if s:
            with torch.cuda.stream(s):
                out.fill_(7.0)
            done = SO.busy(s, SO.busy_ms(), writes)
        else:
            for dst, src in writes:
                dst.copy_(src)
            out.fill_(7.0)
            torch.cuda.synchronize()
        ctx._check(ctx.lib.me_extract_depth_u8(ctx.handle, p(inp), batch, p(fn), p(out), p(fov)))
        if s:
            running = SO.still_running(done)
            d, f = SO.snapshot(s, out), (SO.snapshot(s, fov) if fov is not None else None)
            s.synchronize()
            assert running, ("the producer had finished before the call returned", cfg_name, batch, form, graph, i)
        else:
            ctx.synchronize()
            d, f = out.clone(), (fov.clone() if fov is not None else None)
            torch.cuda.synchronize()
        got.append((d, f))
    assert ctx.graph_launch_count - g0 == (2 if graph else 0), (cfg_name, batch, form, graph, where)
    # eager calls and the capture run the step's host code, a replay does not
    assert ctx.side_branch_count - b0 == ((2 if graph else 3) if want_branch else 0), (ctx.side_branch_count - b0, graph, want_branch)
    ctx.set_graph(False)
    ctx.set_stream(None)
    if not graph and where == "own":
        # the synchronised eager calls on the own stream: what every other combination of this process must reproduce, and what
        # the parent compares over the three processes
        for i in range(PICTURES):
            assert bool(torch.isfinite(got[i][0]).all()) and not bool((got[i][0] == 7.0).all())
            for j in range(i):
                assert not torch.equal(got[i][0], got[j][0]), "two pictures with one result: stale data could pass"
        base[(cfg_name, batch, form)] = got
        key = SO.side_branch_key(cfg_name, batch, form, graph, where)
        saved[key + ".depth"] = torch.stack([d for d, _ in got]).cpu().numpy()
        if fov is not None:
            saved[key + ".fov"] = torch.stack([f for _, f in got]).cpu().numpy()
    else:
        for i, ((d, f), (bd, bf)) in enumerate(zip(got, base[(cfg_name, batch, form)])):
            assert torch.equal(d, bd), ("depth differs from the synchronised eager call", cfg_name, batch, form, graph, where, i)
            assert f is None or torch.equal(f, bf), ("fov differs from the synchronised eager call", cfg_name, batch, form, graph, where, i)
for ctx in ctxs.values():
    ctx.close()
np.savez(path, **saved)
print("side branch ok")
"""


def test_side_branch_changes_no_bit(tmp_path):
    """ME_OVERLAP_TAIL is read once per process: one child with the switch unset, one with it set, one with
    ME_OVERLAP_CAP=8 beside it.  Each runs the tiny and the 8-grid configuration, batch 1 and 2, f_norm given and from the
    FOV head, three eager calls and eager / captured / replayed, on the own stream (synchronised) and on a caller's stream
    (between producer and consumer), and asserts that the branch really ran (me_side_branch_count) or did not.  The three
    calls of a combination run three pictures through the same buffers, so a call never finds its own results in the
    workspaces.  Within a child every combination reproduces the synchronised eager calls on the own stream bit for bit; those
    agree bit for bit over the three children."""
    tests = os.path.dirname(os.path.abspath(__file__))
    base = {k: v for k, v in os.environ.items() if k not in ("ME_OVERLAP_TAIL", "ME_OVERLAP_CAP")}
    outs = {}
    for name, extra in SO.SIDE_BRANCH_ENVS:           # one after the other
        path = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, "-c", _SIDE_BRANCH_CHILD, ROOT, tests, path], env=dict(base, **extra),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "side branch ok" in r.stdout, name + ": " + r.stdout[-2000:] + r.stderr[-3000:]
        outs[name] = dict(np.load(path))
    first = outs["off"]
    assert len(first) == len(SO.SIDE_BRANCH_RUNS) // 4 * 3 // 2       # a depth per (configuration, batch, form), a fov per FOV form
    for name, got in outs.items():
        assert sorted(got) == sorted(first), name
        for key, value in first.items():
            assert np.array_equal(got[key], value), (name, key)


# ---- 5. two contexts at once ----------------------------------------------------------------------------------------------

STEPS = 5


class _Solo:
    """A context of its own, STEPS pictures and the depth of each from synchronised calls on the own stream"""

    def __init__(self, dtype, head0, weights=None, seed=11):
        cfg = m.ModelConfig.tiny()
        cfg.head_dims = (head0, 1)
        self.ctx = m.Context(0, dtype, cfg)
        self.ctx.load_state_dict(weights if weights is not None else (weights_for("tiny") if head0 == 32 else synthetic_checkpoint(cfg)))
        S = cfg.img_size
        self.real = torch.from_numpy(synthetic_images(STEPS, S, "structured", seed=seed)).cuda()
        self.inp = torch.empty_like(self.real)
        self.fn = torch.ones(1, device="cuda")
        self.outs = torch.empty(STEPS, 1, S, S, device="cuda")
        self.stream = torch.cuda.Stream()
        self.inp.copy_(self.real)
        for i in range(STEPS):
            _synced(self.ctx, lambda: self.step(i))
        self.solo = self.outs.clone()
        self.ctx.status_flags()
        self.ctx.set_stream(self.stream.cuda_stream)

    def step(self, i):
        _call_step(self.ctx, "u8", self.inp[i:i + 1], 1, self.fn, self.outs[i], None)

    def producer(self, calls_behind):
        _fill7([self.outs], self.stream)
        return SO.busy(self.stream, SO.busy_ms(calls_behind), [(self.inp, self.real)])

    def finish(self):
        got = SO.snapshot(self.stream, self.outs)
        self.stream.synchronize()
        return got

    def close(self):
        self.ctx.close()


@pytest.fixture()
def pair():
    a, b = _Solo("f16", 32), _Solo("bf16", 16, seed=12)
    yield a, b
    a.close()
    b.close()


def test_two_contexts_one_thread(pair):
    """A (f16, tiny) and B (bf16, head_dims (16, 1)), each on its own caller stream: five steps each, queued alternately
    behind the two producers, nothing synchronised until the end"""
    a, b = pair
    da, db = a.producer(2 * STEPS), b.producer(2 * STEPS)
    for i in range(STEPS):
        a.step(i)
        b.step(i)
    running = SO.still_running(da), SO.still_running(db)
    got_a, got_b = a.finish(), b.finish()
    assert all(running), f"the producers had finished before the steps were queued: {running}"
    assert torch.equal(got_a, a.solo) and torch.equal(got_b, b.solo)
    assert a.ctx.status_flags() == 0 and b.ctx.status_flags() == 0


def test_two_contexts_two_host_threads(pair):
    """The same with one host thread per context (ctypes releases the GIL inside a call): the process-wide tables of gemm.hip
    and the thread-local status word and profiler are entered from two threads at once"""
    a, b = pair
    da, db = a.producer(2 * STEPS), b.producer(2 * STEPS)
    errors = []

    def work(solo):
        try:
            for i in range(STEPS):
                solo.step(i)
        except Exception as e:                               # reported by the test's own thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(x,)) for x in (a, b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    running = SO.still_running(da), SO.still_running(db)
    got_a, got_b = a.finish(), b.finish()
    assert not errors, errors
    assert all(running), f"the producers had finished before the steps were queued: {running}"
    assert torch.equal(got_a, a.solo) and torch.equal(got_b, b.solo)
    assert a.ctx.status_flags() == 0 and b.ctx.status_flags() == 0


def test_status_word_and_destroy_do_not_cross_contexts():
    """A holds the overflowing checkpoint of test_f16_overflow_is_reported_not_swallowed: its steps raise
    ME_STATUS_OVERFLOW_16BIT, B's status stays 0 and B's depth is its solo depth; then A is destroyed while B has steps
    queued behind a running producer, and B's results are intact."""
    w = dict(weights_for("tiny"))
    w["encoder.upsample_latent0.0.weight"] = torch.as_tensor(w["encoder.upsample_latent0.0.weight"]).float() * 3.0e5
    a, b = _Solo("f16", 32, weights=w), _Solo("bf16", 16, seed=12)
    try:
        da, db = a.producer(2 * STEPS), b.producer(2 * STEPS)
        for i in range(STEPS):
            a.step(i)
            b.step(i)
        running = SO.still_running(da), SO.still_running(db)
        got_a, got_b = a.finish(), b.finish()
        assert all(running), f"the producers had finished before the steps were queued: {running}"
        assert torch.equal(got_b, b.solo) and torch.equal(got_a, a.solo)
        assert b.ctx.status_flags() == 0
        assert a.ctx.status_flags() == 1 and a.ctx.status_flags() == 0
        db = b.producer(STEPS)
        for i in range(STEPS):
            b.step(i)
        running = SO.still_running(db)
        a.close()                                            # ... while B's steps wait behind their producer
        got_b = b.finish()
        assert running, "B's producer had finished before A was destroyed"
        assert torch.equal(got_b, b.solo) and b.ctx.status_flags() == 0
    finally:
        a.close()
        b.close()
