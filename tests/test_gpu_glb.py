"""The .glb mesh writer on the GPU (-m gpu): csrc/glb_format.hip through me_mesh_glb_bytes and me_output_mesh(".glb"), byte
for byte against tests/glb_cases.py glb_bytes (an independent restatement of the format) fed from the oracle chain
clamp_minmax -> mesh_index -> mesh_vertices -- flat maps around one 16-byte unit and one workgroup of units, a map whose
isolated far pixel drops out, the scenes of tests/test_gpu_ply.py, non-square maps, all three modes, colours as host arrays
and device tensors, the empty asset, a full 1536 x 1536 mesh once; a cross-check against the PLY writer that needs no
twin; the refusal of a bound that is not finite; the files, the host serialiser as A/B, write-behind, determinism, and
both command lines."""
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
from util import ctx_for, run_cli, tiny_checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glb_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "matrix-eyes_amd", "matrix-eyes-hip")
MODES = {"plain": m.VertexMode.Plain, "color": m.VertexMode.Color, "texture": m.VertexMode.Texture}
SOURCE = "photos/in put.jpg"
# name -> (vertices, faces) on the oracle.  Flat maps keep every vertex: 4 (one unit of colours, three of positions),
# 256 and 255 (around a multiple of 4 and of a workgroup's 256 units), 257 from 258 pixels (one drops out); the scenes
# are those of tests/test_gpu_ply.py; two non-square maps, transposes of each other.
MAPS = {"flat2x2": (4, 2), "flat16x16": (256, 450), "flat17x15": (255, 448), "far43x6": (257, 414),
        "scene16": (66, None), "scene17": (55, None), "scene48": (1792, None), "scene160": (25367, None), "scene257": (65407, None),
        "flat24x40": (960, 1794), "flat40x24": (960, 1794)}
SCENES = {"scene16": (16, 1), "scene17": (17, 3), "scene48": (48, 8), "scene160": (160, 20), "scene257": (257, 259)}


def _ctx():
    return ctx_for("tiny", "f16")


def _scene(shape, seed):
    """tests/test_gpu_ply.py's maps: smooth background + a few nearer rectangles"""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, rows, dtype=np.float32), np.linspace(0, 1, cols, dtype=np.float32), indexing="ij")
    d = 0.2 + 0.15 * np.sin(3 * xx + 2 * yy) + 0.1 * yy
    n = min(rows, cols)
    for _ in range(6):
        x0, y0 = rng.integers(0, n - n // 4, size=2)
        w, h = rng.integers(n // 16, n // 4, size=2)
        d[y0:y0 + h, x0:x0 + w] += rng.uniform(0.2, 1.5)
    d += rng.normal(0, 0.002, size=d.shape).astype(np.float32)
    return np.ascontiguousarray(d.astype(np.float32))


def _depth(name):
    if name in SCENES:
        n, seed = SCENES[name]
        return _scene((n, n), seed)
    rows, cols = (int(v) for v in name.lstrip("flatr").split("x"))
    d = np.full((rows, cols), 0.7, np.float32)
    if name.startswith("far"):
        d[20, 3] = 0.004            # one pixel 250 units away among pixels 1.4 away: every triangle at it is dropped
    return d


def _size(name):
    """the original size: non-square for every map"""
    rows, cols = _depth(name).shape
    return (3 * rows, 2 * cols) if rows == cols else (5 * rows + 1, 3 * cols)


def _pixels(shape, seed=5):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


def _vertex_colors(vi, nv, pixels):
    c = np.zeros((nv, 3), np.uint8)
    c[vi[vi >= 0]] = pixels.reshape(-1, 3)[vi >= 0]
    return c


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(uv, xyz, faces, vertex index, vertex count) of the oracle chain, computed once per map and left unchanged"""
    od, _, _ = OO.clamp_minmax(_depth(name))
    vi, nv, faces = OO.mesh_index(od)
    uv, xyz = OO.mesh_vertices(od, vi, nv, _size(name))
    for a in (uv, xyz, faces, vi):
        a.setflags(write=False)
    return uv, xyz, faces, vi, nv


def _want(name, mode, pixels, source=SOURCE):
    uv, xyz, faces, vi, nv = _oracle(name)
    return G.glb_bytes(xyz, uv, faces, mode, _vertex_colors(vi, nv, pixels) if pixels is not None else None, source)


def test_restatement_passes_its_checker():
    uv, xyz, faces, vi, nv = _oracle("scene17")
    got = G.check_glb(_want("scene17", "color", _pixels((17, 17))))
    assert np.array_equal(got["positions"], G.written_positions(xyz)) and np.array_equal(got["indices"], faces)


@pytest.mark.parametrize("mode", ["plain", "color", "nocolor", "texture"])
@pytest.mark.parametrize("name", list(MAPS))
def test_mesh_glb_bytes_equals_the_restatement(name, mode):
    """the file from host arrays and from device tensors; "nocolor": colour mode without a colour array (no COLOR_0)"""
    ctx = _ctx()
    d = _depth(name)
    uv, xyz, faces, vi, nv = _oracle(name)
    verts, nfaces = MAPS[name]
    assert (verts is None or nv == verts) and (nfaces is None or len(faces) == nfaces) and nv > 0
    pixels = _pixels(d.shape) if mode == "color" else None
    vmode = MODES["color" if mode == "nocolor" else mode]
    want = _want(name, "color" if mode == "nocolor" else mode, pixels)
    got = m.DepthMap(ctx, d, _size(name)).mesh_glb_bytes(SOURCE, vmode, pixels)
    assert len(got) == len(want)
    assert got == want
    parsed = G.check_glb(got)
    assert (parsed["colors"] is not None) == (mode == "color") and (parsed["uvs"] is not None) == (mode == "texture")
    if mode == "texture":
        assert np.array_equal(parsed["uvs"], uv) and parsed["json"]["images"] == [{"uri": SOURCE}]
    od, _, _ = OO.clamp_minmax(d)
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(od.copy()).cuda(), _size(name))
    dev = ddm.mesh_glb_bytes(SOURCE, vmode, torch.from_numpy(pixels).cuda() if pixels is not None else None)
    assert dev.cpu().numpy().tobytes() == want


@pytest.mark.parametrize("name", list(MAPS))
def test_glb_and_ply_hold_the_same_mesh(name):
    """no twin: the PLY file of the same call decodes to the same positions (its f64 are widened f32, so they narrow
    exactly), faces and colours, and the .glb is well formed"""
    ctx = _ctx()
    d = _depth(name)
    pixels = _pixels(d.shape)
    dm = m.DepthMap(ctx, d, _size(name))
    ply = dm.mesh_ply_bytes(m.VertexMode.Color, pixels)
    glb = G.check_glb(dm.mesh_glb_bytes(SOURCE, m.VertexMode.Color, pixels))
    head = ply[:ply.index(b"end_header\n") + 11]
    nv, nf = len(glb["positions"]), len(glb["indices"])
    assert b"element vertex %d\n" % nv in head and b"element face %d\n" % nf in head
    vrec = np.frombuffer(ply, np.dtype([("p", ">f8", 3), ("c", np.uint8, 3)]), nv, len(head))
    frec = np.frombuffer(ply, np.dtype([("n", np.uint8), ("i", ">u4", 3)]), nf, len(head) + 27 * nv)
    assert len(head) + 27 * nv + 13 * nf == len(ply)
    assert np.array_equal(vrec["p"].astype(np.float32).astype(np.float64), vrec["p"])
    assert np.array_equal(vrec["p"].astype(np.float32).view(np.uint32), glb["positions"].view(np.uint32))
    assert np.array_equal(vrec["c"], glb["colors"][:, :3]) and np.array_equal(frec["i"], glb["indices"])


def test_empty_meshes_are_an_asset_without_geometry(tmp_path):
    ctx = _ctx()
    board = np.where(np.add.outer(np.arange(16), np.arange(16)) % 2 == 0, 0.1, 1.0).astype(np.float32)
    smooth = np.array([[0.2, 0.3], [0.5, 0.9]], np.float32)
    empty = G.glb_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), "plain")
    assert len(empty) == 120 and b"BIN" not in empty and G.check_glb(empty)["json"]["scenes"] == [{"nodes": []}]
    for d in (smooth, board):
        od, _, _ = OO.clamp_minmax(d)
        _, nv, faces = OO.mesh_index(od)
        assert nv == 0 and len(faces) == 0
        dm = m.DepthMap(ctx, d, d.shape)
        for mode, pixels in ((m.VertexMode.Plain, None), (m.VertexMode.Color, _pixels(d.shape)), (m.VertexMode.Texture, None)):
            assert dm.mesh_glb_bytes(SOURCE, mode, pixels) == empty
    dm.output_mesh(str(tmp_path / "empty.glb"), SOURCE, m.VertexMode.Plain)
    assert (tmp_path / "empty.glb").read_bytes() == empty


def test_source_path_is_escaped():
    ctx = _ctx()
    source = 'dir "q"\\sub\tphoto \u00e9\u4e2d.jpg'
    got = m.DepthMap(ctx, _depth("flat2x2"), _size("flat2x2")).mesh_glb_bytes(source, m.VertexMode.Texture)
    assert got == _want("flat2x2", "texture", None, source) and G.check_glb(got)["json"]["images"] == [{"uri": source}]


def test_a_bound_that_is_not_finite_is_refused(tmp_path):
    """me_mesh_glb_bytes takes the depth as it is: a flat map of an f32 subnormal has z = 1 / depth = inf and keeps every
    face.  ME_ERR_BAD_ARG and no file; the PLY writer, which can hold inf, still writes it"""
    ctx = _ctx()
    sub = np.array([1], np.uint32).view(np.float32)[0]
    d = np.full((5, 4), sub, np.float32)
    vi, nv, faces = OO.mesh_index(d)
    assert nv == 20 and len(faces) == 24
    ptr, n = C.c_void_p(), C.c_int64()
    args = (ctx.handle, C.c_void_p(d.ctypes.data), 5, 4, 5, 4)
    assert ctx.lib.me_mesh_glb_bytes(*args, b"p.jpg", 0, None, C.byref(ptr), C.byref(n)) == 1
    assert b"not finite" in ctx.lib.me_last_error(ctx.handle)
    dest = tmp_path / "inf.glb"
    assert ctx.lib.me_output_mesh(*args, str(dest).encode(), b"p.jpg", 0, None) == 1 and not dest.exists()
    assert ctx.lib.me_mesh_ply_bytes(*args, 0, None, C.byref(ptr), C.byref(n)) == 0 and n.value > 20 * 24
    good = np.full((5, 4), 0.5, np.float32)      # and the context goes on
    assert ctx.lib.me_mesh_glb_bytes(ctx.handle, C.c_void_p(good.ctypes.data), 5, 4, 5, 4, b"p.jpg", 0, None, C.byref(ptr), C.byref(n)) == 0


def test_full_size_once():
    """a flat map at 1536 x 1536 in colour mode: every vertex, every face, 94 MB; the colour section starts beyond 2^24
    bytes and the index section beyond 2^25 (unit numbers beyond 2^21, more units than one pass of the grid holds)"""
    ctx = _ctx()
    n = 1536
    d = np.full((n, n), 0.7, np.float32)
    vi, nv, faces = OO.mesh_index(d)
    uv, xyz = OO.mesh_vertices(d, vi, nv, (n, n))
    assert nv == n * n == 2359296 and len(faces) == 2 * (n - 1) * (n - 1) == 4712450
    pixels = _pixels((n, n), 6)
    want = np.frombuffer(G.glb_bytes(xyz, uv, faces, "color", _vertex_colors(vi, nv, pixels), SOURCE), np.uint8)
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(d).cuda(), (n, n))
    got = ddm.mesh_glb_bytes(SOURCE, m.VertexMode.Color, torch.from_numpy(pixels).cuda())
    assert got.numel() == len(want) and len(want) > 16 * nv + 12 * len(faces) > 2 ** 26
    got = got.cpu().numpy()
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])


_HOST_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import matrix_eyes_amd as m
z = np.load(sys.argv[2])
ctx = m.Context(0, "f16", m.ModelConfig.tiny())
dm = m.DepthMap(ctx, z["depth"], (160, 160))
for name, mode in (("plain", m.VertexMode.Plain), ("color", m.VertexMode.Color), ("texture", m.VertexMode.Texture)):
    import ctypes as C
    colors = z["pixels"] if name == "color" else None
    ctx._check(ctx.lib.me_output_mesh(ctx.handle, C.c_void_p(dm.data.ctypes.data), 160, 160, 160, 160,
                                      (sys.argv[3] + "/host_" + name + ".glb").encode(), b"photo.jpg", int(mode),
                                      C.c_void_p(colors.ctypes.data) if colors is not None else None))
"""


def _output_mesh(ctx, depth, n, path, mode, colors):
    """me_output_mesh itself: depth and colours as host arrays or device tensors"""
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr() if torch.is_tensor(a) else a.ctypes.data)  # noqa: E731
    return ctx.lib.me_output_mesh(ctx.handle, p(depth), n, n, n, n, str(path).encode(), b"photo.jpg", int(mode), p(colors))


def test_output_mesh_glb_files(tmp_path):
    """the file is me_mesh_glb_bytes' bytes, ".glb" in either letter case, colours as a host array and as a device tensor;
    me_last_mesh_timing reports the call; the host serialiser (ME_GLB_HOST_FORMAT=1, a child process) writes the same"""
    ctx = _ctx()
    n = 160
    d = _depth("scene160")
    dm = m.DepthMap(ctx, d, (n, n))
    pixels = _pixels((n, n))
    want = {"plain": dm.mesh_glb_bytes("photo.jpg", m.VertexMode.Plain), "color": dm.mesh_glb_bytes("photo.jpg", m.VertexMode.Color, pixels),
            "texture": dm.mesh_glb_bytes("photo.jpg", m.VertexMode.Texture)}
    assert len({len(w) for w in want.values()}) == 3
    assert _output_mesh(ctx, dm.data, n, tmp_path / "plain.glb", m.VertexMode.Plain, None) == 0
    assert (tmp_path / "plain.glb").read_bytes() == want["plain"]
    t = ctx.last_mesh_timing()
    assert t["bytes"] == len(want["plain"]) and t["format_ms"] > 0 and min(t["mesh_ms"], t["d2h_ms"], t["file_ms"]) >= 0
    for name, colors in (("host", pixels), ("device", torch.from_numpy(pixels).cuda())):
        assert _output_mesh(ctx, dm.data, n, tmp_path / f"color_{name}.GLB", m.VertexMode.Color, colors) == 0
        assert (tmp_path / f"color_{name}.GLB").read_bytes() == want["color"]
        assert ctx.last_mesh_timing()["bytes"] == len(want["color"])
    assert _output_mesh(ctx, torch.from_numpy(dm.data).cuda(), n, tmp_path / "dev.Glb", m.VertexMode.Texture, None) == 0
    assert (tmp_path / "dev.Glb").read_bytes() == want["texture"]
    assert not list(tmp_path.glob("*.mtl"))
    # the Python mirror's dispatch on the suffix
    dm.output_image(str(tmp_path / "mirror.glb"), "photo.jpg", m.ImageOutputFormat.DepthMap(), m.VertexMode.Texture)
    assert (tmp_path / "mirror.glb").read_bytes() == want["texture"]
    # any other suffix is still refused
    assert _output_mesh(ctx, dm.data, n, tmp_path / "x.gltf", m.VertexMode.Plain, None) == 1
    assert b".obj, .ply or .glb" in ctx.lib.me_last_error(ctx.handle)
    np.savez(tmp_path / "in.npz", depth=d, pixels=pixels)
    r = subprocess.run([sys.executable, "-c", _HOST_CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path)],
                       env=dict(os.environ, ME_GLB_HOST_FORMAT="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in want:
        assert (tmp_path / f"host_{name}.glb").read_bytes() == want[name], name


def test_write_behind_glb(tmp_path):
    """five .glb meshes through the two alternating buffers equal their synchronous files after me_output_flush; a write
    that fails is reported by the flush, once; without write-behind by the call itself"""
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    n = 160
    depths = [m.DepthMap(ctx, _scene((n, n), 20 + i), (n, n)).data for i in range(5)]
    pixels = [_pixels((n, n), 30 + i) for i in range(5)]
    for i in range(5):
        assert _output_mesh(ctx, depths[i], n, tmp_path / f"sync{i}.glb", m.VertexMode.Color, pixels[i]) == 0
    want = [(tmp_path / f"sync{i}.glb").read_bytes() for i in range(5)]
    assert len(set(want)) == 5
    ctx.set_write_behind(True)
    for i in range(5):
        assert _output_mesh(ctx, depths[i], n, tmp_path / f"behind{i}.glb", m.VertexMode.Color, pixels[i]) == 0
    ctx.output_flush()
    for i in range(5):
        assert (tmp_path / f"behind{i}.glb").read_bytes() == want[i]
    assert _output_mesh(ctx, depths[0], n, "/nonexistent-dir/x.glb", m.VertexMode.Plain, None) == 0
    assert ctx.lib.me_output_flush(ctx.handle) == 7 and b"write-behind" in ctx.lib.me_last_error(ctx.handle)
    assert ctx.lib.me_output_flush(ctx.handle) == 0          # reported once
    ctx.set_write_behind(False)
    assert _output_mesh(ctx, depths[0], n, "/nonexistent-dir/x.glb", m.VertexMode.Plain, None) == 7
    assert _output_mesh(ctx, depths[0], n, tmp_path / "again.glb", m.VertexMode.Color, pixels[0]) == 0
    assert (tmp_path / "again.glb").read_bytes() == want[0]


def test_determinism():
    ctx = _ctx()
    d = _depth("scene257")
    dm = m.DepthMap(ctx, d, (257, 257))
    pixels = _pixels(d.shape)
    first = dm.mesh_glb_bytes(SOURCE, m.VertexMode.Color, pixels)
    assert dm.mesh_glb_bytes(SOURCE, m.VertexMode.Color, pixels) == first


def test_command_lines_write_the_same_glb(tmp_path):
    """the compiled command line and the Python one, tiny synthetic checkpoint, a non-square photo: the same vertex-coloured
    and the same textured .glb, each well formed; the texture names the photo as it was given"""
    from PIL import Image
    from matrix_eyes_amd.synthetic import synthetic_images
    assert os.path.exists(CLI), "the compiled command line is built by __graft_entry__.build()"
    S = m.ModelConfig.tiny().img_size
    ckpt, src = str(tmp_path / "tiny.pt"), str(tmp_path / "photo.png")
    tiny_checkpoint(ckpt)
    Image.fromarray(synthetic_images(1, S, "structured", seed=11)[0]).resize((S + 88, S - 40)).save(src)
    env = dict(os.environ, MATRIX_EYES_MODEL="tiny", MATRIX_EYES_SEED="7", MATRIX_EYES_RESAMPLER="device", PYTHONPATH=ROOT)
    files = {}
    for which, argv in (("compiled", [CLI]), ("python", [sys.executable, "-m", "matrix_eyes_amd"])):
        for mesh in ("vertex-colors", "texture-coordinates"):
            dst = tmp_path / f"{which}_{mesh}.glb"
            run_cli(argv + [f"--checkpoint-path={ckpt}", "--focal-length=35", f"--mesh={mesh}", src, str(dst)], env)
            files[which, mesh] = dst.read_bytes()
    for mesh in ("vertex-colors", "texture-coordinates"):
        assert files["compiled", mesh] == files["python", mesh] and len(files["python", mesh]) > 1000, mesh
    assert G.check_glb(files["python", "vertex-colors"])["colors"] is not None
    assert G.check_glb(files["python", "texture-coordinates"])["json"]["images"] == [{"uri": src}]
