"""CPU tests of the keyed stereogram noise: the known answers of the definition, csrc/chacha.h as a
stand-alone program under the sanitizers, the 20-round variant against openssl, the host twin of the library against the
plain-Python restatement tests/chacha_ref.py, the MATRIX_EYES_NOISE switch of the Python mirror and the null pointers."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chacha_ref as R  # noqa: E402

import matrix_eyes_amd as m  # noqa: E402
from matrix_eyes_amd import _lib as L  # noqa: E402
from matrix_eyes_amd import depth_pro as DP  # noqa: E402
from matrix_eyes_amd import output as OUT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_KEY = bytes(32)
COUNT_KEY = bytes(range(32))
COUNTERS = (0, 1, 2**32 - 1, 2**32, 2**32 + 1)
# the definition's known answers
ZERO_BLOCK0 = "9bf49a6a0755f953811fce125f2683d50429c3bb49e074147e0089a52eae155f"
KEY_SEED_0 = "ecf273f981b5cd4587f0467306ad6cadd0d0a3e33317e767f29bea72d78a7dfe"
KEY_SEED_99 = "920f027fbfba66eb3c72467aad13d8ec9b75c98a17c233e8383962181fe214d0"
STREAM_SEED_99 = "9c0217fd090a9da1346a76c1f65193b28a79dc6288c1c739d21ae3d1d45f9cd8"
FIRST_PIXELS = [(0x9b, 0xf4, 0x9a), (0x07, 0x55, 0xf9), (0x81, 0x1f, 0xce), (0x5f, 0x26, 0x83)]


def _key_from_seed(lib, seed):
    buf = (C.c_uint8 * 32)()
    assert lib.me_noise_key_from_seed(seed, buf) == 0
    return bytes(buf)


def _noise_host(lib, key, w, h):
    out = np.empty((h, w, 3), np.uint8)
    assert lib.me_stereogram_noise_host(key, w, h, C.c_void_p(out.ctypes.data)) == 0
    return out


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_restatement():
    assert R.block_bytes(ZERO_KEY, 0)[:32].hex() == ZERO_BLOCK0
    assert [tuple(p) for p in R.noise(ZERO_KEY, 4, 1)[0].tolist()] == FIRST_PIXELS
    assert R.key_from_seed(0).hex() == KEY_SEED_0 and R.key_from_seed(99).hex() == KEY_SEED_99
    assert R.keystream(R.key_from_seed(99), 32).hex() == STREAM_SEED_99


def test_known_answers_of_the_library(lib):
    assert _key_from_seed(lib, 0).hex() == KEY_SEED_0 and _key_from_seed(lib, 99).hex() == KEY_SEED_99
    assert _key_from_seed(lib, 2**64 - 1) == R.key_from_seed(2**64 - 1)
    assert [tuple(p) for p in _noise_host(lib, ZERO_KEY, 4, 1)[0].tolist()] == FIRST_PIXELS
    # the first 32 keystream bytes of seed 99 are the first eight pixels' words: their three low bytes
    stream = bytes.fromhex(STREAM_SEED_99)
    want = [tuple(stream[4 * i:4 * i + 3]) for i in range(8)]
    assert [tuple(p) for p in _noise_host(lib, bytes.fromhex(KEY_SEED_99), 8, 1)[0].tolist()] == want


def test_key_from_os_gives_fresh_keys(lib):
    a, b = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
    assert lib.me_noise_key_from_os(a) == 0 and lib.me_noise_key_from_os(b) == 0
    assert bytes(a) != bytes(b) and bytes(a) != ZERO_KEY


# ---- the header as a stand-alone program, under the sanitizers ---------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chacha_host") / "chacha_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "chacha_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("key", [ZERO_KEY, COUNT_KEY, bytes.fromhex(KEY_SEED_99)], ids=["zero", "count", "seed99"])
def test_the_header_as_a_program_equals_the_restatement(program, key):
    r = subprocess.run([program, key.hex()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [line.split() for line in r.stdout.splitlines()]
    blocks = {(int(f[1]), int(f[2])): f[3] for f in lines if f[0] == "block"}
    assert set(blocks) == {(rounds, c) for rounds in (12, 20) for c in COUNTERS}
    for (rounds, c), got in blocks.items():
        assert got == R.block_bytes(key, c, rounds).hex(), (rounds, c)
    seeds = {int(f[1]): f[2] for f in lines if f[0] == "seed"}
    assert seeds == {s: R.key_from_seed(s).hex() for s in (0, 99, 2**64 - 1)}
    pictures = {(int(f[1]), int(f[2])): f[3] for f in lines if f[0] == "noise"}
    assert pictures == {(w, h): R.noise(key, w, h).tobytes().hex() for w, h in ((17, 2), (5, 3))}


def test_the_header_is_plain():
    text = open(os.path.join(ROOT, "matrix-eyes_amd", "csrc", "chacha.h")).read()
    assert [line for line in text.splitlines() if line.startswith("#include")] == ["#include <stdint.h>"]
    assert "asm" not in text


# ---- the 20-round variant against openssl -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [ZERO_KEY, COUNT_KEY], ids=["zero", "count"])
def test_twenty_rounds_equal_openssl(program, key):
    openssl = shutil.which("openssl")
    if openssl is None:
        pytest.skip("no openssl binary on the path")
    r = subprocess.run([openssl, "enc", "-chacha20", "-K", key.hex(), "-iv", "00" * 16], input=bytes(256), capture_output=True)
    assert r.returncode == 0 and len(r.stdout) == 256, r.stderr
    assert R.keystream(key, 256, rounds=20) == r.stdout
    out = subprocess.run([program, key.hex()], capture_output=True, text=True).stdout
    blocks = {int(f[2]): f[3] for f in (line.split() for line in out.splitlines()) if f[0] == "block" and f[1] == "20"}
    assert bytes.fromhex(blocks[0] + blocks[1]) == r.stdout[:128]


# ---- the host twin of the library against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (16, 1), (17, 2), (255, 3), (1000, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_restatement(lib, size):
    w, h = size
    key = R.key_from_seed(99)
    got = _noise_host(lib, key, w, h)
    assert np.array_equal(got, R.noise(key, w, h))
    if w % 16 and h > 1:      # row 1 starts in the middle of a block: its first pixel is word w & 15 of block w >> 4
        word = R.block_words(key, w >> 4)[w & 15]
        assert tuple(got[1, 0]) == (word & 255, (word >> 8) & 255, (word >> 16) & 255)


# ---- the switch of the Python mirror ------------------------------------------------------------------------------------------
def test_switch_parsing(monkeypatch):
    monkeypatch.delenv("MATRIX_EYES_NOISE", raising=False)
    assert DP.resolve_noise_source() == "legacy"
    for name in ("legacy", "host", "device"):
        monkeypatch.setenv("MATRIX_EYES_NOISE", name)
        assert DP.resolve_noise_source() == name
        assert DP.resolve_noise_source("host") == "host"        # an argument wins over the environment
    for bad in ("fpga", "", "Device"):
        monkeypatch.setenv("MATRIX_EYES_NOISE", bad)
        with pytest.raises(m.MatrixEyesError) as e:
            DP.resolve_noise_source()
        assert e.value.code == 1 and "noise source" in e.value.message and "legacy, host, device" in e.value.message
    with pytest.raises(m.MatrixEyesError):
        DP.resolve_noise_source("numpy")


def test_command_line_mirror_refuses_a_bad_switch(monkeypatch, capsys):
    from matrix_eyes_amd import cli
    monkeypatch.setenv("MATRIX_EYES_NOISE", "fpga")
    assert cli.main(["in.png", "out.png"]) == 2
    assert "MATRIX_EYES_NOISE" in capsys.readouterr().err


class _NoContext:
    """what DepthMap._stereogram_noise needs of a context: the library"""

    def __init__(self, lib):
        self.lib = lib


def _depth_map(lib, size):
    dm = OUT.DepthMap.__new__(OUT.DepthMap)
    dm.ctx = _NoContext(lib)
    dm.original_width, dm.original_height = size
    return dm


def _pointed(ptr, w, h):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(h, w, 3))


def test_legacy_with_a_seed_gives_todays_bytes(lib, monkeypatch):
    monkeypatch.setenv("MATRIX_EYES_SEED", "7")
    w, h = 37, 5
    want = np.random.default_rng(7).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    for env in (None, "legacy"):
        if env is None:
            monkeypatch.delenv("MATRIX_EYES_NOISE", raising=False)
        else:
            monkeypatch.setenv("MATRIX_EYES_NOISE", env)
        gw, gh, ptr, key, keep = _depth_map(lib, (w, h))._stereogram_noise(None, None)
        assert (gw, gh) == (w, h) and key is None
        assert np.array_equal(_pointed(ptr, w, h), want)


def test_host_and_device_take_the_seeds_key(lib, monkeypatch):
    monkeypatch.setenv("MATRIX_EYES_SEED", "18446744073709551615")       # the full 64 bits
    w, h = 37, 5
    key = R.key_from_seed(2**64 - 1)
    _, _, ptr, kbuf, keep = _depth_map(lib, (w, h))._stereogram_noise(None, None, "host")
    assert kbuf is None and np.array_equal(_pointed(ptr, w, h), R.noise(key, w, h))
    _, _, ptr, kbuf, keep = _depth_map(lib, (w, h))._stereogram_noise(None, None, "device")
    assert ptr is None and bytes(kbuf) == key                            # no noise buffer exists: the key goes down
    # a caller's key wins over the seed; a caller's noise wins over everything
    _, _, ptr, kbuf, keep = _depth_map(lib, (w, h))._stereogram_noise(None, None, "device", key=COUNT_KEY)
    assert bytes(kbuf) == COUNT_KEY
    mine = np.full((h, w, 3), 9, np.uint8)
    _, _, ptr, kbuf, keep = _depth_map(lib, (w, h))._stereogram_noise(None, mine, "device")
    assert kbuf is None and np.array_equal(_pointed(ptr, w, h), mine)
    for bad in ("18446744073709551616", "-1", "seven", "0x10"):
        monkeypatch.setenv("MATRIX_EYES_SEED", bad)
        with pytest.raises(m.MatrixEyesError) as e:
            DP.noise_key(lib)
        assert e.value.code == 1 and "MATRIX_EYES_SEED" in e.value.message
    monkeypatch.delenv("MATRIX_EYES_SEED")
    assert len(DP.noise_key(lib)) == 32 and DP.noise_key(lib) != DP.noise_key(lib)     # from the OS
    with pytest.raises(m.MatrixEyesError):
        DP.noise_key(lib, b"short")


# ---- null pointers ------------------------------------------------------------------------------------------------------------
def test_null_pointers_are_bad_arguments(lib):
    BAD_ARG, BAD_SHAPE = 1, 2
    out = np.zeros((2, 2, 3), np.uint8)
    po = C.c_void_p(out.ctypes.data)
    assert lib.me_noise_key_from_seed(1, None) == BAD_ARG
    assert b"me_noise_key_from_seed" in lib.me_last_error(None)
    assert lib.me_noise_key_from_os(None) == BAD_ARG
    assert lib.me_stereogram_noise_host(None, 2, 2, po) == BAD_ARG
    assert lib.me_stereogram_noise_host(ZERO_KEY, 2, 2, None) == BAD_ARG
    assert b"me_stereogram_noise_host" in lib.me_last_error(None)
    assert lib.me_stereogram_noise_host(ZERO_KEY, 0, 2, po) == BAD_SHAPE and lib.me_stereogram_noise_host(ZERO_KEY, 2, -1, po) == BAD_SHAPE
    assert not out.any()                                                # nothing was written
    # the entries that take a context refuse a missing one before anything else
    d = np.full((2, 2), 0.5, np.float32)
    pd = C.c_void_p(d.ctypes.data)
    assert lib.me_stereogram_noise(None, ZERO_KEY, 2, 2, po) == BAD_ARG
    assert lib.me_stereogram_keyed(None, pd, 2, 2, 0.1, 1.0, 2, 2, 0.0625, ZERO_KEY, po) == BAD_ARG
    assert lib.me_stereogram_keyed_dev_range(None, pd, 2, 2, None, 2, 2, 0.0625, ZERO_KEY, po) == BAD_ARG
    assert lib.me_output_stereogram_png_keyed(None, pd, 2, 2, 0.1, 1.0, 2, 2, 0.0625, ZERO_KEY, b"x.png") == BAD_ARG
    assert lib.me_output_stereogram_jpeg_keyed(None, pd, 2, 2, 0.1, 1.0, 2, 2, 0.0625, ZERO_KEY, 75, 2, b"x.jpg") == BAD_ARG
    assert lib.me_last_stereogram_noise(None, None, None) == BAD_ARG
    assert not os.path.exists("x.png") and not os.path.exists("x.jpg")
