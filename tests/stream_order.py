"""Helpers of the stream-order tests (test_gpu_stream_order.py): a producer that keeps the CALLER's stream busy and writes
the real input last, the check that it was still running when the library had finished queuing, and a consumer queued
on the caller's stream right behind the library call.  No host wait separates the three; a test that lets the GPU drain
in between proves nothing about ordering.

The pure-Python part (the calibration arithmetic, the poison fills, the case tables) is held by test_stream_order_cpu.py.
torch is imported by the functions that need it, so the tables can be read without it."""
import math

# Measured on an MI355X, time.perf_counter around the ctypes call, median of 20 warm calls (the largest of 20 in brackets):
# the host time from entering to leaving a device-pointer me_extract_depth on the tiny configuration, eager, is 0.31 ms at
# batch 1 (0.39) and 0.36 ms at batch 2 through the u8 entry with the FOV head (0.50); the 8-grid fp8 configuration takes
# 0.35 ms (0.45).  The call that captures and instantiates the step's hipGraph takes 0.27 ms (0.32), a replay 0.03 ms.  One
# tiny step is 1.3 ms of GPU time at batch 1 and 1.9 ms at batch 2 (8-grid fp8, batch 2: 2.2 ms).
QUEUE_MS_EAGER = 0.36
QUEUE_MS_CAPTURE = 0.27
TINY_STEP_MS = 1.9


def busy_ms_for(queue_ms: float, step_ms: float = TINY_STEP_MS) -> float:
    """The least the producer must run: four times the host time of the call(s) queued behind it, at least one tiny step"""
    if queue_ms <= 0 or step_ms <= 0:
        raise ValueError(f"busy_ms_for({queue_ms}, {step_ms})")
    return max(4.0 * queue_ms, step_ms)


# The rule asks for max(4 * 0.36, 1.9) = 1.9 ms.  The producer runs 10 ms: the rule is a floor (a longer producer hides
# nothing: the library's work waits longer behind it), and 1.9 ms would turn one scheduling hiccup of the host thread
# between busy() and the end of the library call into a failed still_running.
BUSY_MS = 10.0


def busy_ms(calls_behind: int = 1) -> float:
    """BUSY_MS, or what the rule asks for when `calls_behind` steps are queued behind one producer, if that is longer"""
    return max(BUSY_MS, busy_ms_for(calls_behind * max(QUEUE_MS_EAGER, QUEUE_MS_CAPTURE)))

# the matmul chain: square f32 matrices of this side, the count calibrated once per session around this many of them
SCRATCH_SIDE = 2048
CALIBRATION_MATMULS = 64


def matmul_count(ms: float, calib_count: int, calib_ms: float) -> int:
    """Matmuls that take about `ms` when `calib_count` of them took `calib_ms`: rounded up, never none"""
    if ms < 0 or calib_count <= 0 or not calib_ms > 0:
        raise ValueError(f"matmul_count({ms}, {calib_count}, {calib_ms})")
    return max(1, math.ceil(ms * calib_count / calib_ms))


def poison_(t):
    """The fill the producer starts with, in place: NaN for f32 / 16-bit operands; for u8 images, where every byte is a
    valid pixel, the inverted picture 255 - x of what the buffer held (set `t` to the real picture first): another valid
    picture that differs in every byte.  fp8 operand bytes (u8 too) take the same rule."""
    import torch
    if t.dtype == torch.uint8:
        t.bitwise_not_()
    elif t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        raise TypeError(f"poison_: {t.dtype}")
    return t


# ---- case tables -------------------------------------------------------------------------------------------------------
# The step on the caller's stream: (context dtype, model configuration, batch, entry, f_norm form).  An ME_DTYPE_FP8 context
# needs embed_dim % 256 == 0, which the tiny configuration (128) is not: it runs the 8-grid configuration of
# test_captured_graph_replays_the_eager_step.
GRID8 = dict(grid=8, embed_dim=256, num_heads=4, depth=4, tap_blocks=(1, 2), enc_dims=(64, 128, 128, 128), dec_dim=256,
             head_dims=(32, 1))
STEP_CASES = [(dtype, cfg, batch, entry, form)
              for dtype, cfg in (("f16", "tiny"), ("fp8", "grid8"))
              for batch in (1, 2)
              for entry in ("f32", "u8")
              for form in ("f_norm", "fov")]

# The side branch: one child process per environment; every child runs every (configuration, batch, f_norm form, graph,
# stream) combination and saves depth and FOV under the combination's name.
SIDE_BRANCH_ENVS = [("off", {}), ("tail", {"ME_OVERLAP_TAIL": "1"}), ("tail_cap8", {"ME_OVERLAP_TAIL": "1", "ME_OVERLAP_CAP": "8"})]
SIDE_BRANCH_RUNS = [(cfg, batch, form, graph, stream)
                    for cfg in ("tiny", "grid8")
                    for batch in (1, 2)
                    for form in ("f_norm", "fov")
                    for graph in (False, True)
                    for stream in ("own", "caller")]


def side_branch_key(cfg, batch, form, graph, stream) -> str:
    return f"{cfg}.b{batch}.{form}.{'graph' if graph else 'eager'}.{stream}"


# The first launch on a stream nobody has seen: the multi-round shape of test_linear_persistent_rounds and its tile ids
FIRST_LAUNCH_SHAPE = (20195, 1024, 256)
FIRST_LAUNCH_TILES = (0, 1, 3)


# ---- the GPU half --------------------------------------------------------------------------------------------------------
_CALIBRATION = None
_OPERANDS = None      # x and w: read-only, shared by every stream
_SCRATCH = {}         # stream handle -> y, the one tensor a chain writes


def _scratch(stream):
    """(x, w, y): the chain is y = x . w over and over; only y, 16 MB, is per stream (torch hands out at most 32 pool streams)"""
    global _OPERANDS
    import torch
    if _OPERANDS is None:
        _OPERANDS = (torch.rand(SCRATCH_SIDE, SCRATCH_SIDE, device="cuda"), torch.eye(SCRATCH_SIDE, device="cuda"))
        torch.cuda.synchronize()
    key = stream.cuda_stream
    if key not in _SCRATCH:
        _SCRATCH[key] = torch.empty_like(_OPERANDS[0])
        torch.cuda.synchronize()
    return _OPERANDS + (_SCRATCH[key],)


def release():
    """Frees the chain's tensors (the end of the test module that used them)"""
    global _OPERANDS
    _OPERANDS = None
    _SCRATCH.clear()


def calibration():
    """(count, ms) of the fixed matmul chain between two torch events, measured once per session (after a warm-up that
    takes the library's set-up out of it)"""
    global _CALIBRATION
    if _CALIBRATION is None:
        import torch
        s = torch.cuda.Stream()
        x, w, y = _scratch(s)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            for _ in range(8):
                torch.mm(x, w, out=y)
            t0.record(s)
            for _ in range(CALIBRATION_MATMULS):
                torch.mm(x, w, out=y)
            t1.record(s)
        s.synchronize()
        _CALIBRATION = (CALIBRATION_MATMULS, float(t0.elapsed_time(t1)))
    return _CALIBRATION


def busy(stream, ms, writes=()):
    """Keeps `stream` busy for about `ms` with plain torch work and returns a torch event recorded behind it.  writes:
    (destination, real input) pairs.  Every destination is poisoned first (poison_), the LAST ops queued copy the real
    inputs over the poison: a reader that is not ordered behind the whole chain sees the poison."""
    import torch
    count = matmul_count(ms, *calibration())
    x, w, y = _scratch(stream)
    with torch.cuda.stream(stream):
        for dst, src in writes:
            if dst.dtype == torch.uint8:
                dst.copy_(src)
            poison_(dst)
        for _ in range(count):
            torch.mm(x, w, out=y)
        for dst, src in writes:
            dst.copy_(src)
        done = torch.cuda.Event()
        done.record(stream)
    return done


def still_running(event) -> bool:
    """Whether the producer behind which `event` was recorded has not finished: asked right after the library call has
    returned, it says that the library finished queuing while its input did not exist yet"""
    return not event.query()


def snapshot(stream, tensor):
    """The consumer: a copy of `tensor` queued on the caller's stream right behind the library call.  The host then waits
    for that stream only."""
    import torch
    with torch.cuda.stream(stream):
        return tensor.clone()
