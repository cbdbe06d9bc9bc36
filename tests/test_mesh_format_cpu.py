"""CPU tests of the mesh files' host serialisers and of the OBJ line slots: csrc/mesh_host_format.h -- what me_output_mesh runs
under ME_OBJ_HOST_FORMAT=1 / ME_PLY_HOST_FORMAT=1 -- over csrc/obj_format.h's format_line (the text the kernels of
obj_format.hip run) and csrc/ply_format.h's records, compiled as plain C++ (tests/mesh_format_host.cpp) under the address and
undefined-behaviour sanitizers.  Whole files against oracle.output_oracle.obj_text / mtl_text / ply_bytes on the oracle chain of
two scenes of tests/test_gpu_ply.py and on the empty mesh; every line of the worst-case inputs formatted into a heap buffer of
exactly its slot size (kSlotVt / kSlotV / kSlotF, the LDS bytes a kernel thread formats it into without a bound check)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_cases as P  # noqa: E402
from oracle import output_oracle as OO  # noqa: E402
from output_cases import _depth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "mesh_format_host.cpp")
CSRC = os.path.join(ROOT, "matrix-eyes_amd", "csrc")
MODES = ("plain", "color", "texture")
SCENES = {(16, 1): 66, (48, 8): 1792}      # (n, seed) -> vertices, as in tests/test_gpu_ply.py SCENES (the same maps)
SLOT_VT, SLOT_V, SLOT_F = 136, 264, 72     # obj_format.h


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    for h in ("mesh_host_format.h", "obj_format.h", "ply_format.h", "ryu_f64.h"):
        assert os.path.exists(os.path.join(CSRC, h))
    exe = str(tmp_path_factory.mktemp("mesh_format_san") / "mesh_format_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, cases, tmp_path):
    """cases: [(dest, source, mode, uv, xyz, rgb or None, faces, exact_slots)] -> (file, .mtl path, .mtl text) of each"""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "files.bin")
    with open(src, "wb") as f:
        f.write(np.int64(len(cases)).tobytes())
        for dest, source, mode, uv, xyz, rgb, faces, exact in cases:
            assert len(uv) == len(xyz)
            f.write(np.array([MODES.index(mode), len(xyz), len(faces), rgb is not None, exact, len(dest.encode()),
                              len(source.encode())], np.int64).tobytes())
            f.write(dest.encode() + source.encode())
            f.write(np.ascontiguousarray(uv, np.float32).tobytes())
            f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
            if rgb is not None:
                f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
            f.write(np.ascontiguousarray(faces, np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    blob = open(dst, "rb").read()
    blobs, at = [], 0
    for _ in range(3 * len(cases)):
        n = int(np.frombuffer(blob, np.int64, 1, at)[0])
        blobs.append(blob[at + 8:at + 8 + n])
        at += 8 + n
    assert at == len(blob)
    return [tuple(blobs[3 * k:3 * k + 3]) for k in range(len(cases))]


def _scene(n, seed):
    """the oracle chain of tests/test_gpu_ply.py on a non-square original size, and per-vertex colours"""
    od, _, _ = OO.clamp_minmax(_depth(n, seed))
    vi, nv, faces = OO.mesh_index(od)
    uv, xyz = OO.mesh_vertices(od, vi, nv, (3 * n, 2 * n))
    pixels = np.random.default_rng(5).integers(0, 256, size=(n, n, 3), dtype=np.uint8)
    rgb = np.zeros((nv, 3), np.uint8)
    rgb[vi[vi >= 0]] = pixels.reshape(-1, 3)[vi >= 0]
    assert nv == SCENES[(n, seed)] and len(faces) > 0
    return uv, xyz, faces, rgb


def _want(dest, source, mode, uv, xyz, rgb, faces):
    """(file, .mtl path, .mtl text) from the oracle"""
    stem = os.path.splitext(os.path.basename(dest))[0]
    if dest.lower().endswith(".ply"):
        return OO.ply_bytes(xyz, faces, mode, rgb), b"", b""
    with np.errstate(all="ignore"):
        text = OO.obj_text(uv, xyz, faces, mode, stem, rgb).encode()
    if mode != "texture":
        return text, b"", b""
    return text, os.path.join(os.path.dirname(dest), stem + ".mtl").encode(), OO.mtl_text(source).encode()


def test_whole_files_equal_the_oracle_under_sanitizers(driver_san, tmp_path):
    """plain, colour (with and without a colour array) and texture, .obj and .ply, on both scenes and on the empty mesh;
    the .mtl of a textured OBJ and where it goes (a directory, none, ".")"""
    empty = (np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8))
    cases = []
    for mesh, dests in ((_scene(16, 1), ("out/dir.v2/mesh16.obj", "mesh16.PLY")), (_scene(48, 8), ("./scene.48.OBJ", "a/b.ply")),
                        (empty, ("empty.obj", "e/empty.ply"))):
        uv, xyz, faces, rgb = mesh
        for dest in dests:
            for mode, colors in (("plain", None), ("plain", rgb), ("color", rgb), ("color", None), ("texture", None)):
                cases.append((dest, "photos/in put.jpg", mode, uv, xyz, colors, faces, 0))
    got = run(driver_san, cases, tmp_path)
    for case, g in zip(cases, got):
        dest, source, mode, uv, xyz, colors, faces, _ = case
        assert g == _want(dest, source, mode, uv, xyz, colors if mode == "color" else None, faces), (dest, mode, colors is not None)
    assert got[-10][0] == b"" and got[-6][0] == b"mtllib empty.mtl\nusemtl Textured\n" and len(got[-5][0]) == 200


def _longest(text, prefix):
    return max(len(line) + 1 for line in text.split(b"\n") if line.startswith(prefix))


def test_every_line_fits_its_slot_under_sanitizers(driver_san, tmp_path):
    """Each line formatted into a heap buffer of exactly its slot's size, the bytes the oracle's: +-0, subnormals, +-inf and
    +-FLT_MAX in every coordinate (ply_cases.edge_vertices), the negative smallest subnormal in all three (printed, y and z
    negated: one and three numbers of the longest positional form), every colour value in each channel, face ids of ten
    digits in "a/a" pairs."""
    sub = np.array([1], np.uint32).view(np.float32)[0]
    e = np.concatenate([P.edge_vertices(), np.array([[-sub, -sub, -sub], [-sub, sub, sub]], np.float32)])
    rng = np.random.default_rng(17)
    c = np.arange(256)
    ramp = np.stack([c, c[::-1], (c * 7) % 256], -1).astype(np.uint8)      # every value once in each channel
    rgb = ramp[rng.integers(0, 256, len(e))]
    rgb[:256] = ramp
    rgb[-1] = (3, 6, 7)                      # c / 255 of 20 characters each, on the vertex that prints three negative subnormals
    assert all(len(set(rgb[:, k])) == 256 for k in range(3))
    # texture coordinates: the same edge values (u as it is, 1 - v in f64) and f32 fractions, whose 1 - v has 16 - 17 digits
    uv = e[:, :2].copy()
    uv[300:600] = rng.uniform(0, 1, (300, 2)).astype(np.float32)
    top = 2 ** 31 - 2
    faces = np.array([[top, top, top], [0, top, 9], [top - 1, 99999, top]], np.int32)
    cases = [("edge.obj", "p.jpg", mode, uv, e, rgb if mode == "color" else None, faces, 1) for mode in MODES]
    got = run(driver_san, cases, tmp_path)
    for case, g in zip(cases, got):
        assert g == _want(*case[:3], uv, e, case[5], faces), case[2]
    assert _longest(got[2][0], b"vt ") <= SLOT_VT and _longest(got[2][0], b"f ") == 68 <= SLOT_F
    # "v " + three coordinates of 63 characters + three colours of 20, a space before each but the first, '\n'
    assert _longest(got[1][0], b"v ") == 2 + 3 * 63 + 2 + 3 * 21 + 1 == 257 <= SLOT_V
    # the same lines through the serialiser's own buffers
    assert [g[0] for g in run(driver_san, [c[:7] + (0,) for c in cases], tmp_path)] == [g[0] for g in got]
