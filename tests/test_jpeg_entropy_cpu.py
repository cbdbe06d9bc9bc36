"""CPU tests of the device entropy decoder: csrc/jpeg_entropy.h -- the routines the kernels of csrc/jpeg_entropy.hip are made
of -- compiled as plain C++ (tests/jpeg_entropy_host.cpp) and run thread by thread in the kernels' order must give exactly
the coefficients of the host decoder (decode_jpeg_coefficients) for every sequential file of tests/jpeg_files.py, at the
default subsequence length, at 128 bits and at the smallest admitted one, also under the address and undefined-behaviour
sanitizers and on damaged files, where it may instead decline; plan_jpeg_entropy's segments and refusals; the switch; null
contexts."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_files as J  # noqa: E402
import jpeg_entropy_files as E  # noqa: E402

ROOT = J.ROOT
SOURCES = [os.path.join(ROOT, "tests", "jpeg_entropy_host.cpp"),
           os.path.join(J.PKG, "host", "jpeg_decoder.cpp"),
           os.path.join(J.PKG, "csrc", "jpeg_basis.cpp")]
SMALLEST = 64                       # me_jpeg_entropy::kMinSubseqBits
LENGTHS = (0, 128, SMALLEST)        # 0: the default, 1024
PROGRESSIVE, SCANS, HUFFMAN, SHORT = 1, 2, 3, 13   # matrix_eyes::JpegEntropyDecline


def _build(exe, *extra):
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-o", exe, *SOURCES], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()                      # host_selftest, the yardstick of the damaged files
    assert os.path.exists(J.SELFTEST)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("jpeg_entropy") / "jpeg_entropy_host"))


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("jpeg_entropy_san") / "jpeg_entropy_host_san"),
                  "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, data, tmp_path, bits=0, group=256, name="f"):
    """(returncode, report dict, segments [(begin, end)], stderr)"""
    src = str(tmp_path / (name + ".jpg"))
    with open(src, "wb") as f:
        f.write(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, str(bits), str(group)], capture_output=True, text=True, env=env)
    lines = r.stdout.splitlines()
    rep = dict(kv.split("=", 1) for kv in lines[0].split()) if lines else {}
    segs = [tuple(int(v) for v in s.split("-")) for s in lines[1].split()[1:]] if len(lines) > 1 else []
    return r.returncode, rep, segs, r.stderr


def _all_sequential(exe, tmp_path):
    stuffed = 0
    for name, make in E.sequential_files():
        data = make()
        for bits in LENGTHS:
            rc, rep, _, err = run(exe, data, tmp_path, bits, name=name)
            assert rc == 0, (name, bits, rc, rep, err[-2000:])
            assert rep["where"] == "device" and rep["reason"] == "0" and rep["differ"] == "0", (name, bits, rep)
            assert int(rep["bits"]) == (bits or 1024)
            stuffed += int(rep["stuffed"])
    assert stuffed > 0                                            # FF 00 inside the tested scans
    for name, make in E.progressive_files():
        rc, rep, _, err = run(exe, make(), tmp_path, 0, name=name)
        assert rc == 4 and rep["where"] == "host" and int(rep["reason"]) == PROGRESSIVE, (name, rc, rep, err[-2000:])


def test_twin_equals_the_host_decoder(driver, tmp_path):
    _all_sequential(driver, tmp_path)


def test_twin_equals_the_host_decoder_under_sanitizers(driver_san, tmp_path):
    _all_sequential(driver_san, tmp_path)


def test_many_subsequences_and_workgroups(driver, tmp_path):
    """517x333-s2 at the smallest length: thousands of subsequences, and the workgroup size only groups them"""
    data = dict(J.FILES)["517x333-s2"]()
    rc, rep, _, _ = run(driver, data, tmp_path, SMALLEST, 256)
    assert rc == 0 and int(rep["subseqs"]) >= 3109 and int(rep["workgroups"]) > 1
    assert 1 < int(rep["rounds"]) <= 65536 // SMALLEST + 1         # inside the give-up distance
    rc, rep64, _, _ = run(driver, data, tmp_path, SMALLEST, 64)
    assert rc == 0 and rep64["rounds"] == rep["rounds"] and int(rep64["workgroups"]) > int(rep["workgroups"])


def test_plan_segments(driver, tmp_path):
    """segment j of the plan is the bytes between the j-th RSTn and the next marker"""
    for name in ("restart-rows", "restart-blocks"):
        data = dict(J.FILES)[name]()
        rc, rep, segs, _ = run(driver, data, tmp_path, 0, name=name)
        assert rc == 0
        marks = [m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", data) if m.start() > E.scan_start(data)]
        assert len(marks) >= 3 and len(segs) == len(marks) + 1 == int(rep["segments"])
        assert segs[0][0] == E.scan_start(data)
        for j, at in enumerate(marks):
            assert segs[j][1] == at and segs[j + 1][0] == at + 2
        assert data[segs[-1][1]:segs[-1][1] + 2] == b"\xff\xd9"
        assert [data[at + 1] & 7 for at in marks[:8]] == [j & 7 for j in range(min(8, len(marks)))]
    assert any(b"\xff\x00" in make()[E.scan_start(make()):] for name, make in E.sequential_files()[:4])


def test_plan_declines(driver, tmp_path):
    base = bytearray(E.base())
    # a Kraft sum above 1 in the first Huffman table (the standard luminance DC table: 0.998)
    dht = base.index(b"\xff\xc4")
    over = bytearray(base)
    over[dht + 5] += 1                                             # a code of one bit more ...
    longest = max(i for i in range(16) if over[dht + 5 + i])
    over[dht + 5 + longest] -= 1                                   # ... for one of the longest: as many values as before
    rc, rep, _, _ = run(driver, bytes(over), tmp_path, name="kraft")
    assert rc == 4 and rep["where"] == "host" and int(rep["reason"]) == HUFFMAN, rep
    # two scans: the second one a copy of the first
    sos = base.index(b"\xff\xda")
    twice = bytes(base[:-2]) + bytes(base[sos:])
    rc, rep, _, _ = run(driver, twice, tmp_path, name="twice")
    assert rc == 4 and int(rep["reason"]) == SCANS, rep
    # a scan cut short: declined, or the host's zero-extended coefficients
    rc, rep, _, _ = run(driver, E.truncated(), tmp_path, name="trunc")
    assert (rc == 4 and int(rep["reason"]) == SHORT) or (rc == 0 and rep["differ"] == "0"), (rc, rep)


def test_damaged_files(driver_san, built, tmp_path):
    """the three files the GPU test decodes, through the twin under the sanitizers first"""
    for name, make, host_accepts in E.DAMAGED:
        data = make()
        rc_host, _, err = J.host_decode(data, tmp_path, name=name)
        assert (rc_host == 0) == host_accepts, (name, err)
        rc, rep, _, stderr = run(driver_san, data, tmp_path, name=name)
        assert rc in (0, 4), (name, rc, stderr[-2000:])
        assert rep["host"] == ("0" if host_accepts else "3")
        if rc == 0:
            assert host_accepts and rep["differ"] == "0"
    assert "bad Huffman code" in J.host_decode(E.bad_code(), tmp_path, name="bad")[2]
    assert run(driver_san, E.flipped(), tmp_path, name="flip")[0] == 0      # a valid stream: decoded, not declined


def test_corrupted_files_under_sanitizers(driver_san, built, tmp_path):
    """The fuzz loop of tests/test_jpeg_cpu.py::test_corrupted_files_under_sanitizers, same generator, seeds and kinds, on
    its baseline seeds, restart_rows() and grey() (the progressive seed's draws are made and skipped): the twin's
    coefficients equal the host decoder's, or it declines and the host decoder's outcome -- pixels or words -- stands.
    Never a sanitizer report."""
    rng = np.random.default_rng(77)
    seeds = [J.plain(64, 48, 2, False, 85), J.plain(37, 29, 1, True, 85), J.restart_rows(), J.grey()]
    k = decoded = 0
    for index, base in enumerate(seeds):
        for _ in range(12):
            data = bytearray(base)
            kind = int(rng.integers(0, 3))
            if kind == 0:
                for _ in range(int(rng.integers(1, 6))):
                    data[int(rng.integers(2, len(data)))] = int(rng.integers(0, 256))
            elif kind == 1:
                data = data[:int(rng.integers(4, len(data)))]
            else:
                at = int(rng.integers(2, len(data)))
                data[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8))
            k += 1
            if index == 1:
                continue
            name = f"fuzz{k}"
            rc_host, _, _ = J.host_decode(bytes(data), tmp_path, name=name)
            rc, rep, _, stderr = run(driver_san, bytes(data), tmp_path, name=name)
            assert rc in (0, 4), (name, rc, stderr[-2000:])
            assert (rep["host"] == "0") == (rc_host == 0), (name, rep, rc_host)      # the twin's yardstick is the host decoder
            if rc == 0:
                assert rc_host == 0 and rep["differ"] == "0", (name, rep)
                decoded += 1
    assert decoded > 0


def test_switch_values():
    import matrix_eyes_amd as m
    assert m.depth_pro.resolve_jpeg_entropy(None) in ("host", "device")
    assert m.depth_pro.resolve_jpeg_entropy("device") == "device"
    assert m.depth_pro.resolve_jpeg_entropy("host") == "host"
    with pytest.raises(m.MatrixEyesError):
        m.depth_pro.resolve_jpeg_entropy("gpu")


def test_host_coefficients_through_the_library(lib):
    data = J.plain(64, 48)
    count = (48 + 12 + 12) * 64                                     # 4 x 3 MCUs of 4 luma blocks and 1 + 1 chroma blocks
    coef = np.full(count, 7, np.int16)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert lib.me_op_jpeg_coefficients_host(buf, len(data), C.c_void_p(coef.ctypes.data), count) == 0
    assert coef[0] != 7 and (coef != 0).sum() > 100 and (coef[1:64] != 0).any()
    assert lib.me_op_jpeg_coefficients_host(buf, len(data), C.c_void_p(coef.ctypes.data), count - 64) == -2
    assert lib.me_op_jpeg_coefficients_host(None, 0, C.c_void_p(coef.ctypes.data), count) == -1
    bad = E.bad_code()
    buf = (C.c_uint8 * len(bad)).from_buffer_copy(bad)
    assert lib.me_op_jpeg_coefficients_host(buf, len(bad), C.c_void_p(coef.ctypes.data), count) == -3


def test_null_context_is_rejected(lib):
    data = J.plain(8, 8)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    coef = np.zeros(3 * 64 * 4, np.int16)
    assert lib.me_ctx_set_jpeg_entropy(None, 1) == 1
    assert lib.me_last_jpeg_entropy(None, None, None) == 1
    assert lib.me_op_jpeg_entropy(None, buf, len(data), 0, C.c_void_p(coef.ctypes.data), coef.size) == 1
