"""The pure-Python half of tests/stream_order.py: the calibration arithmetic, the poison fills and the case tables of
test_gpu_stream_order.py.  No GPU."""
import math

import pytest
import torch

import stream_order as SO


def test_matmul_count_scales_the_calibration():
    assert SO.matmul_count(10.0, 64, 10.0) == 64
    assert SO.matmul_count(5.0, 64, 10.0) == 32
    assert SO.matmul_count(10.1, 64, 10.0) == 65             # rounded up: never shorter than asked
    assert SO.matmul_count(0.0, 64, 10.0) == 1 and SO.matmul_count(1e-9, 64, 10.0) == 1
    for ms in (0.3, 3.6, 56.0):
        n = SO.matmul_count(ms, 64, 7.5)
        assert (n - 1) * 7.5 / 64 < ms <= n * 7.5 / 64 + 1e-12
    for bad in ((-1.0, 64, 10.0), (1.0, 0, 10.0), (1.0, 64, 0.0), (1.0, 64, float("nan"))):
        with pytest.raises(ValueError):
            SO.matmul_count(*bad)


def test_busy_length_rule():
    """four times the queuing time of the call behind the producer, never less than one tiny step"""
    assert SO.busy_ms_for(1.0, 2.0) == 4.0 and SO.busy_ms_for(0.25, 2.0) == 2.0 and SO.busy_ms_for(0.5, 2.0) == 2.0
    floor = max(SO.busy_ms_for(SO.QUEUE_MS_EAGER), SO.busy_ms_for(SO.QUEUE_MS_CAPTURE))
    assert floor == max(4 * SO.QUEUE_MS_EAGER, 4 * SO.QUEUE_MS_CAPTURE, SO.TINY_STEP_MS)
    assert SO.BUSY_MS >= floor and SO.busy_ms() == SO.BUSY_MS                # the rule is a floor of the chosen length
    for calls in (1, 3, 7, 10, 100):                                         # ... also with several calls behind one producer
        assert SO.busy_ms(calls) >= max(SO.BUSY_MS, 4 * calls * SO.QUEUE_MS_EAGER, SO.TINY_STEP_MS)
    assert SO.busy_ms(100) == 4 * 100 * SO.QUEUE_MS_EAGER > SO.BUSY_MS
    assert SO.QUEUE_MS_EAGER > 0 and SO.QUEUE_MS_CAPTURE > 0 and SO.TINY_STEP_MS > 0
    with pytest.raises(ValueError):
        SO.busy_ms_for(0.0)


def test_poison_fills():
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        t = torch.arange(12, dtype=torch.float32).to(dtype).reshape(3, 4)
        assert SO.poison_(t) is t and bool(torch.isnan(t.float()).all())
    pic = torch.arange(256, dtype=torch.uint8).repeat(3)
    t = pic.clone()
    SO.poison_(t)
    assert t.dtype == torch.uint8 and bool((t != pic).all())                    # another picture, in every byte
    assert torch.equal(t.int(), 255 - pic.int())
    assert torch.equal(SO.poison_(t), pic)                                      # its own inverse
    with pytest.raises(TypeError):
        SO.poison_(torch.zeros(4, dtype=torch.int32))


def test_case_tables():
    assert len(SO.STEP_CASES) == len(set(SO.STEP_CASES)) == 16
    for dtype, cfg, batch, entry, form in SO.STEP_CASES:
        assert dtype in ("f16", "fp8") and batch in (1, 2) and entry in ("f32", "u8") and form in ("f_norm", "fov")
        assert cfg == ("grid8" if dtype == "fp8" else "tiny")
    assert SO.GRID8["embed_dim"] % 256 == 0 and SO.GRID8["embed_dim"] // SO.GRID8["num_heads"] == 64     # what fp8 needs
    assert [n for n, _ in SO.SIDE_BRANCH_ENVS] == ["off", "tail", "tail_cap8"]
    assert SO.SIDE_BRANCH_ENVS[0][1] == {} and SO.SIDE_BRANCH_ENVS[1][1] == {"ME_OVERLAP_TAIL": "1"}
    assert SO.SIDE_BRANCH_ENVS[2][1] == {"ME_OVERLAP_TAIL": "1", "ME_OVERLAP_CAP": "8"}
    assert len(SO.SIDE_BRANCH_RUNS) == 32
    keys = [SO.side_branch_key(*r) for r in SO.SIDE_BRANCH_RUNS]
    assert len(set(keys)) == 32 and "tiny.b1.f_norm.eager.own" in keys and "grid8.b2.fov.graph.caller" in keys
    assert SO.FIRST_LAUNCH_SHAPE == (20195, 1024, 256) and SO.FIRST_LAUNCH_TILES == (0, 1, 3)
    assert SO.CALIBRATION_MATMULS % 2 == 0 and math.log2(SO.SCRATCH_SIDE).is_integer()
