"""CPU tests of the device PLY writer: csrc/ply_format.h -- the record and workgroup routines the kernel of
csrc/ply_format.hip is made of -- compiled as plain C++ (tests/ply_format_host.cpp) under the address and
undefined-behaviour sanitizers and run workgroup by workgroup, lane by lane, must give exactly the bytes of
oracle.output_oracle.ply_bytes: random meshes with nverts, nfaces in {0, 1, 255, 256, 257, 1000}, plain and colour
records, every residue mod 16 of the header's length; the edge values; the two entry points exist and reject a null
context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_cases as P  # noqa: E402
from oracle import output_oracle as OO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "ply_format_host.cpp")
HEADER = os.path.join(ROOT, "matrix-eyes_amd", "csrc", "ply_format.h")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    assert os.path.exists(HEADER)
    exe = str(tmp_path_factory.mktemp("ply_format_san") / "ply_format_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, cases, tmp_path):
    """cases: [(header bytes, xyz, rgb or None, faces)] -> the file of each"""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "files.bin")
    with open(src, "wb") as f:
        f.write(np.int64(len(cases)).tobytes())
        for header, xyz, rgb, faces in cases:
            f.write(np.array([len(header), len(xyz), len(faces), rgb is not None], np.int64).tobytes())
            f.write(header)
            f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
            if rgb is not None:
                f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
            f.write(np.ascontiguousarray(faces, np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    blob = open(dst, "rb").read()
    files, at = [], 0
    for _ in cases:
        n = int(np.frombuffer(blob, np.int64, 1, at)[0])
        files.append(blob[at + 8:at + 8 + n])
        at += 8 + n
    assert at == len(blob)
    return files


def test_restatement_equals_the_oracle():
    P.check_restatement()


def test_twin_equals_the_oracle_under_sanitizers(driver_san, tmp_path):
    """every (nverts, nfaces) pair, plain and colour, behind headers of every length mod 16: the oracle's header with
    0..15 bytes in front of it, which must come back untouched"""
    cases, want = [], []
    for i, nv in enumerate(P.COUNTS):
        for j, nf in enumerate(P.COUNTS):
            xyz, faces, rgb = P.random_mesh(nv, nf, 100 + 10 * i + j)
            for mode, colors in (("plain", None), ("color", rgb)):
                file = OO.ply_bytes(xyz, faces, mode, colors)
                assert file == P.ply_bytes_fast(xyz, faces, mode, colors)
                header = P.ply_header(nv, nf, mode)
                assert file.startswith(header) and len(file) == len(header) + nv * (27 if colors is not None else 24) + nf * 13
                for pad in range(16):
                    front = bytes([0xA0 + pad]) * pad
                    cases.append((front + header, xyz, colors, faces))
                    want.append(front + file)
    assert {len(c[0]) % 16 for c in cases} == set(range(16))
    got = run(driver_san, cases, tmp_path)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, len(cases[k][0]), len(cases[k][1]), len(cases[k][3]), cases[k][2] is not None)


def test_edge_values_under_sanitizers(driver_san, tmp_path):
    """+-0, f32 subnormals, +-inf and +-FLT_MAX in each coordinate: negation and widening are exact"""
    e = P.edge_vertices()
    none = np.zeros((0, 3), np.int32)
    with np.errstate(all="ignore"):
        want = OO.ply_bytes(e, none, "plain")
    header = P.ply_header(len(e), 0, "plain")
    got = run(driver_san, [(header, e, None, none)], tmp_path)[0]
    assert got == want
    body = np.frombuffer(got[len(header):], ">f8").reshape(-1, 3)
    assert np.signbit(body[:, 1]).sum() == np.signbit(-e[:, 1]).sum() > 0       # -0.0 from 0.0, 0.0 from -0.0
    assert np.isinf(body).any() and (np.abs(body) == 2.0 ** -149).any()


def test_entries_exist_and_reject_a_null_context(lib):
    ptr, n = C.c_void_p(), C.c_int64()
    d = np.zeros((2, 2), np.float32)
    assert lib.me_mesh_ply_bytes(None, C.c_void_p(d.ctypes.data), 2, 2, 2, 2, 0, None, C.byref(ptr), C.byref(n)) == 1
    out = np.zeros(64, np.uint8)
    assert lib.me_op_ply_pack(None, C.c_void_p(d.ctypes.data), None, 1, None, 0, 0, C.c_void_p(out.ctypes.data)) == 1
    assert not out.any()
