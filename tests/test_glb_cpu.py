"""CPU tests of the .glb mesh writer: csrc/glb_format.h in host mode -- the layout, the JSON builder and the per-unit
routines the kernels of csrc/glb_format.hip are made of -- through the one-thread serialiser of csrc/mesh_host_format.h
(what ME_GLB_HOST_FORMAT=1 runs), compiled as a stand-alone program (tests/glb_format_host.cpp) under the address and
undefined-behaviour sanitizers.  Its files must equal tests/glb_cases.py glb_bytes, an independent restatement, for V, F
in {0, 1, 3, 4, 5, 255, 256, 257, 1000} in all three modes, and pass its structural checker; a source path with a quote,
a backslash, a tab and non-ASCII UTF-8; the bounds' text at the edge values; the refusal of a bound that is not finite;
the empty asset; the entry point exists and rejects a null context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glb_cases as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "glb_format_host.cpp")
HEADER = os.path.join(ROOT, "matrix-eyes_amd", "csrc", "glb_format.h")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    assert os.path.exists(HEADER)
    exe = str(tmp_path_factory.mktemp("glb_format_san") / "glb_format_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, cases, tmp_path):
    """cases: [(mode, source, uv, xyz, rgb or None, faces)] -> per case the file, or None when it was refused"""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "files.bin")
    with open(src, "wb") as f:
        f.write(np.int64(len(cases)).tobytes())
        for mode, source, uv, xyz, rgb, faces in cases:
            raw = source.encode()
            f.write(np.array([G.MODES.index(mode), len(xyz), len(faces), rgb is not None, len(raw)], np.int64).tobytes())
            f.write(raw)
            f.write(np.ascontiguousarray(uv, np.float32).tobytes())
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
        refused, n = (int(v) for v in np.frombuffer(blob, np.int64, 2, at))
        files.append(None if refused else blob[at + 16:at + 16 + n])
        at += 16 + n
    assert at == len(blob)
    return files


def test_restatement_passes_its_checker():
    """glb_bytes and check_glb are written apart from each other: the one's files satisfy the other"""
    for nv, nf in ((0, 0), (1, 1), (4, 2), (5, 7), (257, 300)):
        xyz, uv, faces, rgb = G.random_mesh(nv, nf, 3)
        for mode, colors in (("plain", None), ("color", rgb), ("color", None), ("texture", None)):
            got = G.check_glb(G.glb_bytes(xyz, uv, faces, mode, colors, "p.jpg"), referenced=3 * nf >= nv)
            if nv:
                assert np.array_equal(got["positions"], G.written_positions(xyz)) and np.array_equal(got["indices"], faces)
                assert (got["colors"] is not None) == (mode == "color" and colors is not None)
                assert (got["uvs"] is not None) == (mode == "texture")


def test_files_equal_the_restatement_under_sanitizers(driver_san, tmp_path):
    """every (V, F) pair in all three modes, colour mode also without a colour array (no colour section), plain and
    texture mode with an array that must not be read; the empty asset in each mode"""
    cases = []
    for i, nv in enumerate((0,) + G.COUNTS):
        for j, nf in enumerate(G.COUNTS if nv else (0,)):
            xyz, uv, faces, rgb = G.random_mesh(nv, nf, 100 + 10 * i + j)
            for mode, colors in (("plain", None), ("color", rgb), ("color", None), ("texture", rgb if (i + j) % 2 else None)):
                cases.append((mode, "photos/in put.jpg", uv, xyz, colors, faces))
    got = run(driver_san, cases, tmp_path)
    sizes = set()
    for (mode, source, uv, xyz, colors, faces), g in zip(cases, got):
        want = G.glb_bytes(xyz, uv, faces, mode, colors, source)
        assert g == want, (mode, len(xyz), len(faces), colors is not None)
        G.check_glb(g, referenced=3 * len(faces) >= len(xyz))
        sizes.add(len(g) % 16)
    assert len(got[0]) == 120 and got[0] == got[1] == got[2] == got[3]          # the empty asset: JSON alone, any mode
    assert len(sizes) > 1                                                       # files that end inside a 16-byte unit too


def test_source_path_is_escaped(driver_san, tmp_path):
    """a quote, a backslash, a tab, another control byte and non-ASCII UTF-8 in the picture's path: the uri reads back as
    the path, the UTF-8 bytes stand in the file as they are"""
    source = 'dir "q"\\sub\tphoto\x01 \u00e9\u4e2d.jpg'
    xyz, uv, faces, rgb = G.random_mesh(5, 4, 7)
    texture, plain = run(driver_san, [("texture", source, uv, xyz, None, faces), ("plain", source, uv, xyz, None, faces)], tmp_path)
    assert texture == G.glb_bytes(xyz, uv, faces, "texture", None, source)
    assert G.check_glb(texture)["json"]["images"] == [{"uri": source}]
    assert b'"uri":"dir \\"q\\"\\\\sub\\u0009photo\\u0001 \xc3\xa9\xe4\xb8\xad.jpg"' in texture
    assert plain == G.glb_bytes(xyz, uv, faces, "plain", None, source) and b"photo" not in plain


def test_bounds_text_at_the_edge_values(driver_san, tmp_path):
    """zeros of both signs, f32 subnormals and +-FLT_MAX as bounds: min / max are printed as the OBJ writer prints them
    and read back to the data's bounds; -0 is the smaller zero"""
    sub = np.array([1], np.uint32).view(np.float32)[0]
    fmax = np.finfo(np.float32).max
    meshes = [np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]], np.float32),       # written: (0, -0, -0), (-0, 0, 0)
              np.array([[0.0, -0.0, -0.0]], np.float32),                          # written: all +0
              np.array([[sub, -sub, fmax], [-sub, sub, -fmax], [fmax, 1.5, 0.1]], np.float32)]
    cases = [("plain", "", np.zeros((len(x), 2), np.float32), x, None, np.arange(3, dtype=np.int32).reshape(1, 3) % len(x)) for x in meshes]
    got = run(driver_san, cases, tmp_path)
    for (mode, source, uv, xyz, _, faces), g in zip(cases, got):
        assert g == G.glb_bytes(xyz, uv, faces, mode, None, source)
        G.check_glb(g)
    assert b'"min":[-0,-0,-0],"max":[0,0,0]' in got[0] and b'"min":[0,0,0],"max":[0,0,0]' in got[1]
    j = G.check_glb(got[2])["json"]
    assert float(j["accessors"][0]["max"][0]) == float(fmax) and j["accessors"][0]["min"][1] == -1.5
    start = got[2].index(b'"min":[')
    bounds = got[2][start:got[2].index(b"]}", start) + 1]
    assert b"e" not in bounds.lower().replace(b'"max"', b"") and len(bounds) > 150            # positional, never scientific


def test_a_bound_that_is_not_finite_is_refused(driver_san, tmp_path):
    """inf or NaN in any written component, of either sign, anywhere among the vertices: no file"""
    xyz, uv, faces, rgb = G.random_mesh(9, 6, 11)
    cases = []
    for value in (np.inf, -np.inf, np.nan, -np.nan):
        for comp in range(3):
            bad = xyz.copy()
            bad[4 + comp, comp] = value
            cases.append(("color", "p.jpg", uv, bad, rgb, faces))
            with pytest.raises(G.Refused):
                G.glb_bytes(bad, uv, faces, "color", rgb, "p.jpg")
    cases.append(("color", "p.jpg", uv, xyz, rgb, faces))
    got = run(driver_san, cases, tmp_path)
    assert all(g is None for g in got[:-1]) and got[-1] == G.glb_bytes(xyz, uv, faces, "color", rgb, "p.jpg")


def test_entry_exists_and_rejects_a_null_context(lib):
    ptr, n = C.c_void_p(), C.c_int64()
    d = np.zeros((2, 2), np.float32)
    assert lib.me_mesh_glb_bytes(None, C.c_void_p(d.ctypes.data), 2, 2, 2, 2, b"p.jpg", 0, None, C.byref(ptr), C.byref(n)) == 1
    assert not ptr.value and n.value == 0
