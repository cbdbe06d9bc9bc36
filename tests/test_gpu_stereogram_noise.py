"""GPU tests of the keyed stereogram noise: the fill kernel of me_stereogram_noise against the plain-Python
restatement tests/chacha_ref.py, the keyed stereogram entries against me_stereogram fed the host twin's noise and against
the C oracle fed the restatement's, their device-range and file forms, their refusals, and both command lines under
MATRIX_EYES_NOISE.  Array equality everywhere; every case is small."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chacha_ref as R  # noqa: E402
import output_cases as X  # noqa: E402

import matrix_eyes_amd as m  # noqa: E402
from oracle import output_oracle as OO  # noqa: E402
from util import ctx_for, run_cli, tiny_checkpoint  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
BAD_ARG, BAD_SHAPE = 1, 2
KEY = R.key_from_seed(99)
OTHER_KEY = R.key_from_seed(100)
NOISE_SIZES = [(1, 1), (5, 3), (17, 2), (255, 3), (257, 3), (1000, 7), (16384, 2), (1536, 64)]      # (out_w, out_h)
# on the 64x64 map: a whole-row span at the LDS limit, pattern_width 16 at the widest row, blocks that straddle every row start
NEW_CASES = [X.StereoCase("64x64", 16384, 2, X.AMP_BIG), X.StereoCase("64x64", 16384, 2, X.AMP_ZERO),
             X.StereoCase("64x64", 1000, 7, 1.0 / 16.0)]
CASES = {c.name: c for c in X.STEREO_CASES + X.NARROW_CASES + NEW_CASES}
TALL = "96x40-257x3-a0.0625"


def _ctx():
    return ctx_for("tiny", "f16")


def _vp(a):
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def _last_error(ctx):
    return ctx.lib.me_last_error(ctx.handle).decode()


@functools.lru_cache(maxsize=None)
def ref_noise(out_w, out_h, key=KEY):
    n = R.noise(key, out_w, out_h)
    n.setflags(write=False)
    return n


def twin_noise(ctx, out_w, out_h, key=KEY):
    out = np.empty((out_h, out_w, 3), np.uint8)
    assert ctx.lib.me_stereogram_noise_host(key, out_w, out_h, _vp(out)) == 0
    return out


def _last_noise(ctx):
    report, ms = (C.c_int64 * 2)(), C.c_double()
    ctx._check(ctx.lib.me_last_stereogram_noise(ctx.handle, report, C.byref(ms)))
    return report[0], report[1], ms.value


# ---- the fill kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", NOISE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_fill_equals_the_restatement(size):
    w, h = size
    ctx, want = _ctx(), ref_noise(*size)
    host = np.zeros((h, w, 3), np.uint8)
    ctx._check(ctx.lib.me_stereogram_noise(ctx.handle, KEY, w, h, _vp(host)))
    assert np.array_equal(host, want)
    assert _last_noise(ctx)[:2] == (1, (w * h + 15) // 16 * 16)
    # into device memory, with a guard behind the picture; twice: the same bytes
    dev = torch.full((h * w * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        ctx._check(ctx.lib.me_stereogram_noise(ctx.handle, KEY, w, h, _vp(dev)))
        ctx.synchronize()
        got = dev.cpu().numpy()
        assert np.array_equal(got[:h * w * 3].reshape(h, w, 3), want) and np.all(got[h * w * 3:] == 0xA5)
    ctx._check(ctx.lib.me_stereogram_noise(ctx.handle, OTHER_KEY, w, h, _vp(host)))
    assert not np.array_equal(host, want) and np.array_equal(host, ref_noise(w, h, OTHER_KEY))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_noise_fill_into_an_unaligned_slice(offset):
    ctx, (w, h) = _ctx(), (257, 3)
    dev = torch.full((offset + h * w * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx._check(ctx.lib.me_stereogram_noise(ctx.handle, KEY, w, h, C.c_void_p(dev.data_ptr() + offset)))
    ctx.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[offset:offset + h * w * 3].reshape(h, w, 3), ref_noise(w, h))
    assert np.all(got[:offset] == 0xA5) and np.all(got[offset + h * w * 3:] == 0xA5)


# ---- the keyed stereogram -------------------------------------------------------------------------------------------------------
def _keyed(ctx, depth, mn, mx, out_w, out_h, amplitude, key, out):
    return ctx.lib.me_stereogram_keyed(ctx.handle, _vp(depth), depth.shape[0], depth.shape[1], mn, mx, out_w, out_h, amplitude,
                                       key, _vp(out))


def _from_buffer(ctx, depth, mn, mx, out_w, out_h, amplitude, noise, out):
    return ctx.lib.me_stereogram(ctx.handle, _vp(depth), depth.shape[0], depth.shape[1], mn, mx, out_w, out_h, amplitude,
                                 _vp(noise), _vp(out))


@functools.lru_cache(maxsize=None)
def keyed_oracle(name):
    """(rc, out) of the C oracle's stereogram fed the restatement's noise, computed once, read-only"""
    case = CASES[name]
    od, _, _ = X.stereo_map(case.map)
    mn, mx = X.stereo_range(case)
    rc, out, _, _ = OO.stereogram_counted(od, mn, mx, case.out_w, case.out_h, case.amplitude, ref_noise(case.out_w, case.out_h))
    if out is not None:
        out.setflags(write=False)
    return rc, out


@pytest.mark.parametrize("name", list(CASES))
def test_keyed_stereogram_equals_the_buffer_path_and_the_oracle(name):
    case, ctx = CASES[name], _ctx()
    od, _, _ = X.stereo_map(case.map)
    mn, mx = X.stereo_range(case)
    rc, want = keyed_oracle(name)
    assert rc == 0 and od.shape[0] >= od.shape[1]       # as the existing stereogram tests: every case is admitted
    keyed = np.zeros((case.out_h, case.out_w, 3), np.uint8)
    ctx._check(_keyed(ctx, od, mn, mx, case.out_w, case.out_h, case.amplitude, KEY, keyed))
    fed = np.zeros_like(keyed)
    ctx._check(_from_buffer(ctx, od, mn, mx, case.out_w, case.out_h, case.amplitude, twin_noise(ctx, case.out_w, case.out_h), fed))
    assert np.array_equal(keyed, fed)
    assert np.array_equal(keyed, want)


def test_keyed_stereogram_into_device_memory_and_its_report():
    """a device destination; me_last_stereogram_noise names the keyed entry's fill (path 2) and its whole blocks"""
    ctx = _ctx()
    for case in (NEW_CASES[2], NEW_CASES[0]):
        od, mn, mx = X.stereo_map(case.map)
        out = torch.empty((case.out_h, case.out_w, 3), dtype=torch.uint8, device="cuda")
        ctx._check(_keyed(ctx, od, mn, mx, case.out_w, case.out_h, case.amplitude, KEY, out))
        path, words, ms = _last_noise(ctx)
        assert (path, words) == (2, (case.out_w * case.out_h + 15) // 16 * 16) and ms > 0
        assert np.array_equal(out.cpu().numpy(), keyed_oracle(case.name)[1])
    # a different key gives a different picture
    other = np.zeros((7, 1000, 3), np.uint8)
    od, mn, mx = X.stereo_map("64x64")
    ctx._check(_keyed(ctx, od, mn, mx, 1000, 7, 1.0 / 16.0, OTHER_KEY, other))
    assert not np.array_equal(other, keyed_oracle(NEW_CASES[2].name)[1])


# ---- variants on a tall map ------------------------------------------------------------------------------------------------------
def test_keyed_stereogram_with_the_range_on_the_device():
    case, ctx = CASES[TALL], _ctx()
    od, mn, mx = X.stereo_map(case.map)
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(np.array(od)).cuda(), (case.out_w, case.out_h))
    got = ddm.stereogram(case.amplitude, key=KEY)
    assert ddm.inverse_depth_range() == (mn, mx)
    assert np.array_equal(got.cpu().numpy(), keyed_oracle(TALL)[1])
    with pytest.raises(m.MatrixEyesError):
        ddm.stereogram(case.amplitude)      # neither noise nor key


def test_keyed_stereogram_files_of_a_tall_map(tmp_path):
    from PIL import Image
    case, ctx = CASES[TALL], _ctx()
    od, _, _ = X.stereo_map(case.map)
    dm = m.DepthMap(ctx, od, (case.out_w, case.out_h))
    want = keyed_oracle(TALL)[1]
    assert np.array_equal(dm.stereogram(None, case.amplitude, noise_source="device", key=KEY), want)
    assert np.array_equal(dm.stereogram(None, case.amplitude, noise_source="host", key=KEY), want)
    dm.output_stereogram_png(str(tmp_path / "k.png"), None, case.amplitude, noise_source="device", key=KEY)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "k.png")), want)
    dm.output_stereogram_jpeg(str(tmp_path / "k.jpg"), None, case.amplitude, noise_source="device", key=KEY)
    dm.output_stereogram_jpeg(str(tmp_path / "b.jpg"), None, case.amplitude, noise=twin_noise(ctx, case.out_w, case.out_h))
    assert (tmp_path / "k.jpg").read_bytes() == (tmp_path / "b.jpg").read_bytes()


# ---- refusals, as me_stereogram -------------------------------------------------------------------------------------------------
def test_keyed_entries_refuse_what_the_buffer_entries_refuse(tmp_path):
    ctx = _ctx()
    out_w, out_h, amp = 70, 3, 1.0 / 16.0
    out = np.full((out_h, out_w, 3), 0x5A, np.uint8)
    png, jpg = str(tmp_path / "x.png").encode(), str(tmp_path / "x.jpg").encode()

    def entries(depth, rows, cols, mn, mx, w, h, key, range_dev):
        lib, hd = ctx.lib, ctx.handle
        yield lib.me_stereogram_keyed(hd, _vp(depth), rows, cols, mn, mx, w, h, amp, key, _vp(out))
        yield lib.me_output_stereogram_png_keyed(hd, _vp(depth), rows, cols, mn, mx, w, h, amp, key, png)
        yield lib.me_output_stereogram_jpeg_keyed(hd, _vp(depth), rows, cols, mn, mx, w, h, amp, key, 75, 2, jpg)
        if range_dev is not None:
            ddev, odev = torch.from_numpy(np.array(depth)).cuda(), torch.full((h * w * 3,), 0x5A, dtype=torch.uint8, device="cuda")
            yield lib.me_stereogram_keyed_dev_range(hd, _vp(ddev), rows, cols, _vp(range_dev), w, h, amp, key, _vp(odev))
            ctx.synchronize()
            assert bool((odev == 0x5A).all())

    rdev = torch.tensor([0.1, 1.0], dtype=torch.float32, device="cuda")
    # a map with more columns than rows
    wide, mn, mx = X.stereo_map("40x96")
    for rc in entries(wide, 40, 96, mn, mx, out_w, out_h, KEY, rdev):
        msg = _last_error(ctx)
        assert rc == BAD_SHAPE and "40x96" in msg and "rows >= cols" in msg
    # a row wider than 16384, non-positive sizes
    tall, mn, mx = X.stereo_map("96x40")
    for w, h in ((16385, 1), (0, 3), (70, 0), (-1, 3)):
        big = np.full((max(h, 1), max(w, 1), 3), 0x5A, np.uint8)
        assert ctx.lib.me_stereogram_keyed(ctx.handle, _vp(tall), 96, 40, mn, mx, w, h, amp, KEY, _vp(big)) == BAD_SHAPE, (w, h)
        assert ctx.lib.me_output_stereogram_png_keyed(ctx.handle, _vp(tall), 96, 40, mn, mx, w, h, amp, KEY, png) == BAD_SHAPE
        assert ctx.lib.me_output_stereogram_jpeg_keyed(ctx.handle, _vp(tall), 96, 40, mn, mx, w, h, amp, KEY, 75, 2, jpg) == BAD_SHAPE
        assert ctx.lib.me_stereogram_noise(ctx.handle, KEY, w, h, _vp(big)) == BAD_SHAPE
        assert np.all(big == 0x5A)
    assert ctx.lib.me_stereogram_keyed(ctx.handle, _vp(tall), 96, 40, mn, mx, 16385, 1, amp, KEY, _vp(out)) == BAD_SHAPE
    assert "16384" in _last_error(ctx)
    # null pointers
    for rc in entries(tall, 96, 40, mn, mx, out_w, out_h, None, rdev):
        assert rc == BAD_ARG
    assert ctx.lib.me_stereogram_keyed(ctx.handle, None, 96, 40, mn, mx, out_w, out_h, amp, KEY, _vp(out)) == BAD_ARG
    assert ctx.lib.me_stereogram_keyed(ctx.handle, _vp(tall), 96, 40, mn, mx, out_w, out_h, amp, KEY, None) == BAD_ARG
    assert ctx.lib.me_stereogram_keyed_dev_range(ctx.handle, _vp(tall), 96, 40, None, out_w, out_h, amp, KEY, _vp(out)) == BAD_ARG
    assert ctx.lib.me_output_stereogram_png_keyed(ctx.handle, _vp(tall), 96, 40, mn, mx, out_w, out_h, amp, KEY, None) == BAD_ARG
    assert ctx.lib.me_stereogram_noise(ctx.handle, None, out_w, out_h, _vp(out)) == BAD_ARG
    assert ctx.lib.me_stereogram_noise(ctx.handle, KEY, out_w, out_h, None) == BAD_ARG
    assert np.all(out == 0x5A) and os.listdir(tmp_path) == []           # nothing written, no file created
    # the context is still good
    ctx._check(_keyed(ctx, tall, mn, mx, out_w, out_h, amp, KEY, out))
    assert not np.all(out == 0x5A)


# ---- both command lines -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    from PIL import Image
    from matrix_eyes_amd.synthetic import synthetic_images
    assert os.path.exists(CLI), "the compiled command line is built by __graft_entry__.build()"
    d = tmp_path_factory.mktemp("noise_cli")
    S = m.ModelConfig.tiny().img_size
    ckpt, src = str(d / "tiny.pt"), str(d / "photo.png")
    tiny_checkpoint(ckpt)
    Image.fromarray(synthetic_images(1, S, "structured", seed=11)[0]).resize((S + 88, S - 40)).save(src)
    base = dict(os.environ, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_SEED="7", PYTHONPATH=ROOT)
    base.pop("MATRIX_EYES_NOISE", None)
    return d, ckpt, src, base, (S - 40, S + 88, 3)


def _run(which, cli_inputs, noise, dst, expect=0, **more):
    d, ckpt, src, base, _ = cli_inputs
    argv = [CLI] if which == "compiled" else [sys.executable, "-m", "matrix_eyes_amd"]
    env = dict(base, **more) if noise is None else dict(base, MATRIX_EYES_NOISE=noise, **more)
    return run_cli(argv + [f"--checkpoint-path={ckpt}", "--focal-length=35", "--image-output-format=stereogram", src, dst], env, expect)


def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_command_lines_write_the_same_pixels_for_a_seed(cli_inputs):
    """The switch settles the noise; the same picture also needs the same depth map, so both command lines resize the photo
    with the same resampler here (the compiled one's default; the mirror's default, Pillow's filter, is within one code of it
    and can move a shift by a pixel)."""
    d, shape = cli_inputs[0], cli_inputs[4]
    pictures = {}
    for which in ("compiled", "python"):
        for noise in ("host", "device"):
            dst = str(d / f"{which}_{noise}.png")
            _run(which, cli_inputs, noise, dst, MATRIX_EYES_RESAMPLER="device")
            pictures[which, noise] = _pixels(dst)
            assert pictures[which, noise].shape == shape
    first = pictures["compiled", "host"]
    for k, p in pictures.items():
        assert np.array_equal(p, first), (k, int((p != first).any(axis=2).sum()))
    # ... and through the device PNG encoder, whose keyed entry the switch then takes
    dst = str(d / "compiled_device_png.png")
    _run("compiled", cli_inputs, "device", dst, MATRIX_EYES_PNG_ENCODER="device", MATRIX_EYES_RESAMPLER="device")
    assert np.array_equal(_pixels(dst), first)
    # the seed's key decides: the top-left pixels (x < pattern_width) are the noise itself
    pw = X.pattern_width(shape[1], 1.0 / 16.0)
    assert np.array_equal(first[:, :pw], R.noise(R.key_from_seed(7), shape[1], shape[0])[:, :pw])


def test_legacy_noise_is_unchanged_on_both_command_lines(cli_inputs):
    d, ckpt, src, base, shape = cli_inputs
    # the compiled one: the switch unset and "legacy" are the same run, and not the keyed noise
    for name, noise in (("c_unset", None), ("c_legacy", "legacy")):
        _run("compiled", cli_inputs, noise, str(d / f"{name}.png"))
    unset = _pixels(str(d / "c_unset.png"))
    assert np.array_equal(unset, _pixels(str(d / "c_legacy.png")))
    pw = X.pattern_width(shape[1], 1.0 / 16.0)
    assert not np.array_equal(unset[:, :pw], R.noise(R.key_from_seed(7), shape[1], shape[0])[:, :pw])
    # the mirror: its PCG64 draw for the seed, as output.py has always made it
    _run("python", cli_inputs, "legacy", str(d / "p_legacy.png"))
    got = _pixels(str(d / "p_legacy.png"))
    draw = np.random.default_rng(7).integers(0, 256, size=shape, dtype=np.uint8)
    assert np.array_equal(got[:, :pw], draw[:, :pw])
    # a bad value is refused by both before anything is written
    for which, status in (("compiled", 1), ("python", 2)):
        r = _run(which, cli_inputs, "fpga", str(d / "x.png"), expect=status)
        assert "MATRIX_EYES_NOISE" in r.stdout + r.stderr and not (d / "x.png").exists()
