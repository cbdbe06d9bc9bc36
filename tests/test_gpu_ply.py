"""The PLY writer on the GPU (-m gpu): csrc/ply_format.hip through me_op_ply_pack, me_mesh_ply_bytes and
me_output_mesh(".ply"), byte for byte against oracle.output_oracle.ply_bytes (reference output.rs:385-482) -- the record
packing around one workgroup's span and at every residue mod 16 of the header's length, whole meshes against the full
oracle chain, the empty and the smallest mesh, a full 1536 x 1536 mesh once, the files, the host serialiser as A/B,
write-behind and determinism."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from oracle import output_oracle as OO
from util import ctx_for

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"plain": m.VertexMode.Plain, "color": m.VertexMode.Color, "texture": m.VertexMode.Texture}
# (n, seed) -> vertices on the oracle, header length mod 16 (plain, colour), face-section start mod 16 (plain, colour)
SCENES = {(16, 1): (66, (10, 6), (10, 12)), (17, 3): (55, (10, 6), (2, 3)), (48, 8): (1792, (14, 10), (14, 10)),
          (160, 20): (25367, (0, 12), (8, 9)), (257, 259): (65407, (1, 13), (9, 2))}
GUARD = 64


def _ctx():
    return ctx_for("tiny", "f16")


def _depth(n, seed=0, kind="scene"):
    """tests/test_gpu_output.py's maps: smooth background + a few nearer rectangles (discontinuities)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, n, dtype=np.float32), np.linspace(0, 1, n, dtype=np.float32),
                         indexing="ij")
    d = 0.2 + 0.15 * np.sin(3 * xx + 2 * yy) + 0.1 * yy
    if kind == "scene":
        for _ in range(6):
            x0, y0 = rng.integers(0, n - n // 4, size=2)
            w, h = rng.integers(n // 16, n // 4, size=2)
            d[y0:y0 + h, x0:x0 + w] += rng.uniform(0.2, 1.5)
        d += rng.normal(0, 0.002, size=d.shape).astype(np.float32)
    return np.ascontiguousarray(d.astype(np.float32))


def _pixels(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, size=(n, n, 3), dtype=np.uint8)


def _vertex_colors(vi, nv, pixels):
    c = np.zeros((nv, 3), np.uint8)
    c[vi[vi >= 0]] = pixels.reshape(-1, 3)[vi >= 0]
    return c


@functools.lru_cache(maxsize=None)
def _oracle(n, seed, size):
    """(clamped depth, xyz, faces, vertex index, vertex count) of the oracle chain, computed once per scene"""
    od, _, _ = OO.clamp_minmax(_depth(n, seed))
    vi, nv, faces = OO.mesh_index(od)
    _, xyz = OO.mesh_vertices(od, vi, nv, size)
    for a in (od, xyz, faces, vi):
        a.setflags(write=False)
    return od, xyz, faces, vi, nv


def _pack(ctx, xyz, rgb, faces, header_bytes, front):
    """me_op_ply_pack on device tensors -> (bytes in front, body, guard behind)"""
    nv, nf = len(xyz), len(faces)
    body = nv * (27 if rgb is not None else 24) + nf * 13
    out = torch.full((header_bytes + body + GUARD,), front, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()      # torch's fill runs on torch's stream, the kernel on the context's
    ctx._check(ctx.lib.me_op_ply_pack(ctx.handle, C.c_void_p(xyz.data_ptr()) if nv else None,
                                      C.c_void_p(rgb.data_ptr()) if rgb is not None else None, nv,
                                      C.c_void_p(faces.data_ptr()) if nf else None, nf, header_bytes, C.c_void_p(out.data_ptr())))
    ctx.synchronize()
    got = out.cpu().numpy().tobytes()
    return got[:header_bytes], got[header_bytes:header_bytes + body], got[header_bytes + body:]


def test_restatement_equals_the_oracle():
    P.check_restatement()


@pytest.mark.parametrize("colour", [False, True], ids=["plain", "color"])
def test_pack_around_a_workgroup_and_every_residue(colour):
    """nverts, nfaces in {0, 1, 255, 256, 257, 1000} (one workgroup packs 256 records), 24- and 27-byte vertex
    records, header_bytes of every residue mod 16 (torch's allocations are 16-byte aligned, so that is the residue of
    the body's address): the oracle's records, nothing in front of header_bytes or behind the end written."""
    ctx = _ctx()
    for i, nv in enumerate(P.COUNTS):
        for j, nf in enumerate(P.COUNTS):
            xyz, faces, rgb = P.random_mesh(nv, nf, 100 + 10 * i + j)
            want = OO.ply_bytes(xyz, faces, "color" if colour else "plain", rgb if colour else None)
            want = want[len(P.ply_header(nv, nf, "color" if colour else "plain")):]
            assert want == P.ply_body_fast(xyz, faces, rgb if colour else None)
            dx, df = torch.from_numpy(xyz).cuda(), torch.from_numpy(faces).cuda()
            dc = torch.from_numpy(rgb).cuda() if colour else None
            assert dx.data_ptr() % 16 == 0
            for r in range(16):
                header_bytes = 192 + r if (i + j) % 2 else r
                front, body, behind = _pack(ctx, dx, dc, df, header_bytes, 0xA0 + r)
                assert body == want, (nv, nf, header_bytes)
                assert front == bytes([0xA0 + r]) * header_bytes and behind == bytes([0xA0 + r]) * GUARD, (nv, nf, header_bytes)


def test_pack_host_pointers():
    """the same entry on host arrays: the caller's first header_bytes stay as they are"""
    ctx = _ctx()
    xyz, faces, rgb = P.random_mesh(257, 300, 9)
    out = np.full(203 + 257 * 27 + 300 * 13 + GUARD, 0x5A, np.uint8)
    ctx._check(ctx.lib.me_op_ply_pack(ctx.handle, C.c_void_p(xyz.ctypes.data), C.c_void_p(rgb.ctypes.data), 257,
                                      C.c_void_p(faces.ctypes.data), 300, 203, C.c_void_p(out.ctypes.data)))
    got = out.tobytes()
    assert got[:203] == b"\x5a" * 203 and got[-GUARD:] == b"\x5a" * GUARD
    assert got[203:-GUARD] == P.ply_body_fast(xyz, faces, rgb)


def test_pack_edge_values():
    """0.0, -0.0, f32 subnormals, +-inf and +-FLT_MAX in each coordinate: negation and widening are exact"""
    ctx = _ctx()
    e = P.edge_vertices()
    none = np.zeros((0, 3), np.int32)
    with np.errstate(all="ignore"):
        want = OO.ply_bytes(e, none, "plain")[len(P.ply_header(len(e), 0, "plain")):]
    front, body, behind = _pack(ctx, torch.from_numpy(e).cuda(), None, torch.from_numpy(none).cuda(), 7, 0xC3)
    assert body == want and front == b"\xc3" * 7 and behind == b"\xc3" * GUARD
    back = np.frombuffer(body, ">f8").reshape(-1, 3)
    assert np.array_equal(np.signbit(back[:, 1]), np.signbit(-e[:, 1])) and np.signbit(back[:, 1]).any()
    assert np.isinf(back).any() and (np.abs(back) == 2.0 ** -149).any()


@pytest.mark.parametrize("mode", ["plain", "color", "texture"])
@pytest.mark.parametrize("n,seed", sorted(SCENES))
def test_mesh_ply_bytes_equals_the_oracle(n, seed, mode):
    """clamp_minmax -> mesh_index -> mesh_vertices -> ply_bytes, on a non-square original size"""
    ctx = _ctx()
    size = (3 * n, 2 * n)
    od, xyz, faces, vi, nv = _oracle(n, seed, size)
    nverts, head_res, face_res = SCENES[(n, seed)]
    assert nv == nverts
    pixels = _pixels(n) if mode == "color" else None
    want = OO.ply_bytes(xyz, faces, mode, _vertex_colors(vi, nv, pixels) if pixels is not None else None)
    header = P.ply_header(nv, len(faces), mode)
    k = 1 if mode == "color" else 0
    assert len(header) % 16 == head_res[k] and (len(want) - 13 * len(faces)) % 16 == face_res[k]
    got = m.DepthMap(ctx, _depth(n, seed), size).mesh_ply_bytes(MODES[mode], pixels)
    assert len(got) == len(want)
    assert got == want
    if n == 48 and mode != "color":      # even n: vertices at x_norm = 0.5 and y_norm = 0.5, so 0.0 in x and -0.0 in y
        v = np.frombuffer(got[len(header):len(header) + nv * 24], ">f8").reshape(-1, 3)
        assert {int(((v[:, 1] == 0) & np.signbit(v[:, 1])).sum()), int(((v[:, 0] == 0) & ~np.signbit(v[:, 0])).sum())} == {35, 41}


def test_empty_meshes_are_the_header_alone():
    ctx = _ctx()
    board = np.where(np.add.outer(np.arange(16), np.arange(16)) % 2 == 0, 0.1, 1.0).astype(np.float32)
    for d in (_depth(2, 1, "smooth"), board):
        n = d.shape[0]
        od, _, _ = OO.clamp_minmax(d)
        _, nv, faces = OO.mesh_index(od)
        assert nv == 0 and len(faces) == 0
        dm = m.DepthMap(ctx, d, (n, n))
        plain, colour = dm.mesh_ply_bytes(m.VertexMode.Plain), dm.mesh_ply_bytes(m.VertexMode.Color, _pixels(n))
        assert plain == OO.ply_bytes(np.zeros((0, 3), np.float32), faces, "plain") and len(plain) == 200
        assert colour == OO.ply_bytes(np.zeros((0, 3), np.float32), faces, "color", np.zeros((0, 3), np.uint8)) and len(colour) == 260


def test_smallest_full_mesh():
    ctx = _ctx()
    d = np.full((2, 2), 0.7, np.float32)
    od, _, _ = OO.clamp_minmax(d)
    vi, nv, faces = OO.mesh_index(od)
    _, xyz = OO.mesh_vertices(od, vi, nv, (2, 2))
    assert nv == 4 and len(faces) == 2
    pixels = _pixels(2)
    dm = m.DepthMap(ctx, d, (2, 2))
    assert dm.mesh_ply_bytes(m.VertexMode.Plain) == OO.ply_bytes(xyz, faces, "plain")
    assert dm.mesh_ply_bytes(m.VertexMode.Color, pixels) == OO.ply_bytes(xyz, faces, "color", _vertex_colors(vi, nv, pixels))


def test_colour_mode_without_colours():
    """ME_VERTEX_COLOR with vertex_colors == NULL: the colour properties in the header, 24-byte records"""
    ctx = _ctx()
    n, seed = 48, 8
    od, xyz, faces, vi, nv = _oracle(n, seed, (n, n))
    got = m.DepthMap(ctx, _depth(n, seed), (n, n)).mesh_ply_bytes(m.VertexMode.Color, None)
    assert got == OO.ply_bytes(xyz, faces, "color", None)
    assert b"property uchar red" in got[:260] and len(got) == len(P.ply_header(nv, len(faces), "color")) + 24 * nv + 13 * len(faces)


def test_full_size_once():
    """a flat map at 1536 x 1536 in colour mode: every vertex, every face; byte offsets beyond any 16-bit or workgroup-local
    range (125 MB), the size in closed form"""
    ctx = _ctx()
    n = 1536
    d = np.full((n, n), 0.7, np.float32)
    vi, nv, faces = OO.mesh_index(d)
    _, xyz = OO.mesh_vertices(d, vi, nv, (n, n))
    assert nv == n * n == 2359296 and len(faces) == 2 * (n - 1) * (n - 1) == 4712450
    pixels = _pixels(n, 6)
    want = P.ply_bytes_fast(xyz, faces, "color", _vertex_colors(vi, nv, pixels))
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(d).cuda(), (n, n))
    got = ddm.mesh_ply_bytes(m.VertexMode.Color, torch.from_numpy(pixels).cuda())
    assert got.numel() == len(P.ply_header(nv, len(faces), "color")) + 27 * nv + 13 * len(faces) == len(want)
    got = got.cpu().numpy()
    w = np.frombuffer(want, np.uint8)
    assert np.array_equal(got, w), int(np.flatnonzero(got != w)[0])


_HOST_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import matrix_eyes_amd as m
z = np.load(sys.argv[2])
ctx = m.Context(0, "f16", m.ModelConfig.tiny())
dm = m.DepthMap(ctx, z["depth"], (160, 160))
import ctypes as C
for name, mode, colors in (("plain", 0, None), ("color", 1, z["pixels"])):
    ctx._check(ctx.lib.me_output_mesh(ctx.handle, C.c_void_p(dm.data.ctypes.data), 160, 160, 160, 160,
                                      (sys.argv[3] + "/host_" + name + ".ply").encode(), b"photo.jpg", mode,
                                      C.c_void_p(colors.ctypes.data) if colors is not None else None))
"""


def _output_mesh(ctx, depth, n, path, mode, colors):
    """me_output_mesh itself: depth and colours as host arrays or device tensors"""
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr() if torch.is_tensor(a) else a.ctypes.data)  # noqa: E731
    return ctx.lib.me_output_mesh(ctx.handle, p(depth), n, n, n, n, str(path).encode(), b"photo.jpg", int(mode), p(colors))


def test_output_mesh_ply_files(tmp_path):
    """the file is me_mesh_ply_bytes' bytes, with the colours as a host array and as a device tensor;
    me_last_mesh_timing reports the call; the host serialiser (ME_PLY_HOST_FORMAT=1, a child process) writes the same"""
    ctx = _ctx()
    n, seed = 160, 20
    dm = m.DepthMap(ctx, _depth(n, seed), (n, n))
    pixels = _pixels(n)
    want = {"plain": dm.mesh_ply_bytes(m.VertexMode.Plain), "color": dm.mesh_ply_bytes(m.VertexMode.Color, pixels)}
    od, xyz, faces, vi, nv = _oracle(n, seed, (n, n))
    assert want["color"] == OO.ply_bytes(xyz, faces, "color", _vertex_colors(vi, nv, pixels))
    assert _output_mesh(ctx, dm.data, n, tmp_path / "plain.ply", m.VertexMode.Plain, None) == 0
    assert (tmp_path / "plain.ply").read_bytes() == want["plain"]
    t = ctx.last_mesh_timing()
    assert t["bytes"] == len(want["plain"]) and t["format_ms"] > 0 and min(t["mesh_ms"], t["d2h_ms"], t["file_ms"]) >= 0
    for name, colors in (("host", pixels), ("device", torch.from_numpy(pixels).cuda())):
        assert _output_mesh(ctx, dm.data, n, tmp_path / f"color_{name}.PLY", m.VertexMode.Color, colors) == 0
        assert (tmp_path / f"color_{name}.PLY").read_bytes() == want["color"]
        assert ctx.last_mesh_timing()["bytes"] == len(want["color"])
    # a device depth map too
    assert _output_mesh(ctx, torch.from_numpy(dm.data).cuda(), n, tmp_path / "dev.ply", m.VertexMode.Color,
                        torch.from_numpy(pixels).cuda()) == 0
    assert (tmp_path / "dev.ply").read_bytes() == want["color"]
    np.savez(tmp_path / "in.npz", depth=_depth(n, seed), pixels=pixels)
    r = subprocess.run([sys.executable, "-c", _HOST_CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path)],
                       env=dict(os.environ, ME_PLY_HOST_FORMAT="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "host_plain.ply").read_bytes() == want["plain"]
    assert (tmp_path / "host_color.ply").read_bytes() == want["color"]


def test_write_behind_ply(tmp_path):
    """five .ply meshes through the two alternating buffers equal their synchronous files after me_output_flush; a write
    that fails is reported by the flush, once; without write-behind by the call itself"""
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    n = 160
    depths = [m.DepthMap(ctx, _depth(n, seed=20 + i), (n, n)).data for i in range(5)]
    pixels = [_pixels(n, 30 + i) for i in range(5)]
    for i in range(5):
        assert _output_mesh(ctx, depths[i], n, tmp_path / f"sync{i}.ply", m.VertexMode.Color, pixels[i]) == 0
    want = [(tmp_path / f"sync{i}.ply").read_bytes() for i in range(5)]
    assert len(set(want)) == 5
    ctx.set_write_behind(True)
    for i in range(5):
        assert _output_mesh(ctx, depths[i], n, tmp_path / f"behind{i}.ply", m.VertexMode.Color, pixels[i]) == 0
    ctx.output_flush()
    for i in range(5):
        assert (tmp_path / f"behind{i}.ply").read_bytes() == want[i]
    assert _output_mesh(ctx, depths[0], n, "/nonexistent-dir/x.ply", m.VertexMode.Plain, None) == 0
    assert ctx.lib.me_output_flush(ctx.handle) == 7 and b"write-behind" in ctx.lib.me_last_error(ctx.handle)
    assert ctx.lib.me_output_flush(ctx.handle) == 0          # reported once
    ctx.set_write_behind(False)
    assert _output_mesh(ctx, depths[0], n, "/nonexistent-dir/x.ply", m.VertexMode.Plain, None) == 7
    assert _output_mesh(ctx, depths[0], n, tmp_path / "again.ply", m.VertexMode.Color, pixels[0]) == 0
    assert (tmp_path / "again.ply").read_bytes() == want[0]


def test_determinism():
    ctx = _ctx()
    n, seed = 257, 259
    dm = m.DepthMap(ctx, _depth(n, seed), (n, n))
    pixels = _pixels(n)
    first = dm.mesh_ply_bytes(m.VertexMode.Color, pixels)
    assert dm.mesh_ply_bytes(m.VertexMode.Color, pixels) == first
