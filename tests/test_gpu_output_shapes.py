"""Output back end at the shapes and edges of tests/output_cases.py (-m gpu): non-square maps, ragged counts, special values
and the branches no square map enters, through the C ABI, BIT-EXACT against the C oracle (oracle/output_oracle.c).  Everything
here is integer / byte work or f32 arithmetic the oracle fixes bit for bit, so every comparison is array equality -- there is
no tolerance in this file.  Each case was admitted on the CPU (tests/test_output_cases_cpu.py) from the oracle alone.

A depth map with more columns than rows never reaches the stereogram kernel: the library refuses it (ME_ERR_BAD_SHAPE), and the
refusal is what the last tests hold."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import matrix_eyes_amd as m
from oracle import output_oracle as OO
import output_cases as X
from util import ctx_for

pytestmark = pytest.mark.gpu
BAD_SHAPE = 2                       # ME_ERR_BAD_SHAPE
ORIGINAL = (640, 480)               # a non-square picture: x_multiplier != y_multiplier
MODES = {"plain": m.VertexMode.Plain, "color": m.VertexMode.Color, "texture": m.VertexMode.Texture}


def _ctx():
    return ctx_for("tiny", "f16")


def _vp(a):
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


def _last_error(ctx):
    return (ctx.lib.me_last_error(ctx.handle) or b"").decode()


# ---- clamp + range --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", X.CLAMP_CONTENTS)
@pytest.mark.parametrize("count", X.CLAMP_COUNTS)
def test_clamp_minmax_every_path(count, content):
    """me_depth_clamp_minmax on a host and on a device pointer (16-byte accesses + scalar tail), me_depth_clamp_minmax_async on
    a device slice 0 - 3 floats off 16-byte alignment (from 1 on: the all-scalar path): the clamped bits -- NaN signs and
    payloads included -- and (min, max) are the oracle's, and the elements around the slice are not touched."""
    ctx = _ctx()
    d = X.clamp_case(count, content)
    od, mn, mx = X.clamp_oracle(count, content)
    want = od.view(np.uint32)
    a, b = C.c_float(), C.c_float()
    host = d.copy()
    ctx._check(ctx.lib.me_depth_clamp_minmax(ctx.handle, _vp(host), count, C.byref(a), C.byref(b)))
    assert np.array_equal(_bits(host), want) and (a.value, b.value) == (mn, mx)
    dev = torch.from_numpy(d.copy()).cuda()
    assert dev.data_ptr() % 16 == 0
    a, b = C.c_float(), C.c_float()
    ctx._check(ctx.lib.me_depth_clamp_minmax(ctx.handle, _vp(dev), count, C.byref(a), C.byref(b)))
    assert np.array_equal(_bits(dev), want) and (a.value, b.value) == (mn, mx)
    for off in (0, 1, 2, 3):
        buf = torch.full((count + off + 5,), 7.0, dtype=torch.float32, device="cuda")
        sl = buf[off:off + count]
        sl.copy_(torch.from_numpy(d.copy()))
        rng = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0 and sl.data_ptr() % 16 == 4 * off
        ctx._check(ctx.lib.me_depth_clamp_minmax_async(ctx.handle, _vp(sl), count, _vp(rng)))
        ctx.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[off:off + count].view(np.uint32), want), off
        assert (got[:off] == 7.0).all() and (got[off + count:] == 7.0).all(), off
        assert tuple(rng.tolist()) == (mn, mx), off


# ---- mesh -----------------------------------------------------------------------------------------------------------------
def _oracle_vertices(name):
    od, ovi, onv, ofaces = X.mesh_oracle(name)
    ouv, oxyz = OO.mesh_vertices(od, ovi, onv, ORIGINAL)
    return od, ovi, onv, ofaces, ouv, oxyz


@pytest.mark.parametrize("name", [c.name for c in X.MESH_CASES])
def test_mesh_index_and_vertices_on_non_square_maps(name):
    ctx = _ctx()
    case = X.MESH_BY_NAME[name]
    od, ovi, onv, ofaces, ouv, oxyz = _oracle_vertices(name)
    dm = m.DepthMap(ctx, od, ORIGINAL)
    assert np.array_equal(_bits(dm.data), _bits(od))            # the clamp leaves a clamped map alone, NaNs included
    assert (dm.data_width, dm.data_height) == (case.width, case.height)
    vi, nv, faces = dm.mesh_index()
    assert nv == onv and len(faces) == len(ofaces)
    assert np.array_equal(vi, ovi) and np.array_equal(faces, ofaces)
    uv, xyz = dm.mesh_vertices(vi, nv)
    assert np.array_equal(_bits(uv), _bits(ouv)) and np.array_equal(_bits(xyz), _bits(oxyz))
    # counting only (faces == NULL)
    vi2, nv2, nf2 = dm.mesh_index(want_faces=False)
    assert (nv2, nf2) == (onv, len(ofaces)) and np.array_equal(vi2, ovi)


@pytest.mark.parametrize("name", [c.name for c in X.MESH_CASES if c.content == "checker"])
def test_mesh_that_keeps_nothing_writes_no_face(name):
    ctx = _ctx()
    case = X.MESH_BY_NAME[name]
    od, ovi, _, _ = X.mesh_oracle(name)
    w, h = case.width, case.height
    for on_device in (False, True):
        faces = np.full((2 * case.nquads, 3), 0x5a5a5a5a, np.int32)
        vi = np.full((w * h,), 12345, np.int32)
        depth = od
        if on_device:
            faces, vi, depth = (torch.from_numpy(np.array(a)).cuda() for a in (faces, vi, od))
        nv, nf = C.c_int64(-1), C.c_int64(-1)
        ctx._check(ctx.lib.me_mesh_index(ctx.handle, _vp(depth), w, h, _vp(vi), C.byref(nv), C.byref(nf), _vp(faces)))
        ctx.synchronize()
        assert (nv.value, nf.value) == (0, 0)
        assert (_bits(faces) == 0x5a5a5a5a).all()
        assert np.array_equal(vi.cpu().numpy() if on_device else vi, ovi) and (ovi == -1).all()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", X.MESH_FILE_CASES)
def test_mesh_files_on_non_square_maps(tmp_path, name, mode):
    """The device file producers on a non-square map: the OBJ text and the PLY bytes in device memory, and the files
    me_output_mesh writes from the device-resident depth, are the oracle writers' bytes -- a file of no vertex and no face
    (5x7-checker) included."""
    ctx = _ctx()
    od, ovi, onv, ofaces, ouv, oxyz = _oracle_vertices(name)
    colors = vcol = cdev = None
    if mode == "color":
        colors = np.random.default_rng(3).integers(0, 256, size=od.shape + (3,), dtype=np.uint8)
        vcol = np.zeros((onv, 3), np.uint8)
        vcol[ovi[ovi >= 0]] = colors.reshape(-1, 3)[ovi >= 0]
        cdev = torch.from_numpy(colors).cuda()
    want_obj = OO.obj_text(ouv, oxyz, ofaces, mode, "scene", vcol).encode()
    want_ply = OO.ply_bytes(oxyz, ofaces, mode, vcol)
    if onv == 0:        # still well formed: the headers alone
        assert want_obj == (b"mtllib scene.mtl\nusemtl Textured\n" if mode == "texture" else b"")
        assert want_ply.endswith(b"end_header\n") and b"element vertex 0\n" in want_ply and b"element face 0\n" in want_ply
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(od.copy()).cuda(), ORIGINAL)
    assert ddm.obj_text("scene", MODES[mode], cdev).cpu().numpy().tobytes() == want_obj
    assert ddm.mesh_ply_bytes(MODES[mode], cdev).cpu().numpy().tobytes() == want_ply
    ddm.output_mesh(str(tmp_path / "scene.obj"), "photo.jpg", MODES[mode], cdev)
    ddm.output_mesh(str(tmp_path / "scene.ply"), "photo.jpg", MODES[mode], cdev)
    assert (tmp_path / "scene.obj").read_bytes() == want_obj
    assert (tmp_path / "scene.ply").read_bytes() == want_ply
    if mode == "texture":
        assert (tmp_path / "scene.mtl").read_text() == OO.mtl_text("photo.jpg")
    else:
        assert not (tmp_path / "scene.mtl").exists()
    # the host-side mirror takes the same path from a host pointer
    assert m.DepthMap(ctx, od, ORIGINAL).mesh_ply_bytes(MODES[mode], colors) == want_ply


@pytest.mark.parametrize("width,height", [(1, 5), (5, 1), (1, 1), (0, 7)])
def test_mesh_entries_refuse_a_map_without_a_quad(tmp_path, width, height):
    ctx = _ctx()
    d = np.full((5,), 0.5, np.float32)
    vi = np.zeros((8,), np.int32)
    nv, nf, ptr, n = C.c_int64(), C.c_int64(), C.c_void_p(), C.c_int64()
    dest = tmp_path / "none.obj"
    assert ctx.lib.me_mesh_index(ctx.handle, _vp(d), width, height, _vp(vi), C.byref(nv), C.byref(nf), None) == BAD_SHAPE
    assert f"{width}x{height}" in _last_error(ctx)
    assert ctx.lib.me_mesh_obj_text(ctx.handle, _vp(d), width, height, 64, 48, b"scene", 0, None, C.byref(ptr),
                                    C.byref(n)) == BAD_SHAPE
    assert ctx.lib.me_mesh_ply_bytes(ctx.handle, _vp(d), width, height, 64, 48, 0, None, C.byref(ptr),
                                     C.byref(n)) == BAD_SHAPE
    assert ctx.lib.me_output_mesh(ctx.handle, _vp(d), width, height, 64, 48, str(dest).encode(), b"photo.jpg", 0,
                                  None) == BAD_SHAPE
    assert f"{width}x{height}" in _last_error(ctx) and not dest.exists()


# ---- colour map -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", X.COLOUR_CONTENTS)
@pytest.mark.parametrize("shape", X.COLOUR_SHAPES)
def test_depth_map_rgb_on_non_square_maps(shape, content):
    ctx = _ctx()
    d = X.colour_map(shape, content)
    od, mn, mx = OO.clamp_minmax(d)
    dm = m.DepthMap(ctx, d, (shape[1], shape[0]))
    assert np.array_equal(_bits(dm.data), _bits(od)) and dm.inverse_depth_range() == (mn, mx)
    want = OO.depthmap_rgb(od, mn, mx)
    assert np.array_equal(dm.depth_map_rgb(), want)
    # the chained form: range read from device memory
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(d.copy()).cuda(), (shape[1], shape[0]))
    got = ddm.depth_map_rgb()
    # (inverse_depth_range() synchronises the context's stream, which torch's copy back to the host does not wait for: first)
    assert ddm.inverse_depth_range() == (mn, mx) and np.array_equal(got.cpu().numpy(), want)


# ---- stereogram -------------------------------------------------------------------------------------------------------------
def _raw_stereogram(ctx, depth, mn, mx, out_w, out_h, amplitude, noise, out):
    return ctx.lib.me_stereogram(ctx.handle, _vp(depth), depth.shape[0], depth.shape[1], mn, mx, out_w, out_h, amplitude,
                                 _vp(noise), _vp(out))


@pytest.mark.parametrize("name", [c.name for c in X.STEREO_CASES + X.NARROW_CASES])
def test_stereogram_on_tall_maps_and_edge_sizes(name):
    """me_stereogram with explicit (min_depth, max_depth): the map's own range, or -- the narrow cases -- one that makes pixels
    refer forward, to noise the row has not overwritten yet"""
    ctx = _ctx()
    case = X.STEREO_BY_NAME[name]
    od, _, _ = X.stereo_map(case.map)
    mn, mx = X.stereo_range(case)
    rc, want, _, _ = X.stereo_oracle(name)
    assert rc == 0 and od.shape[0] >= od.shape[1]
    out = np.full((case.out_h, case.out_w, 3), 0xa5, np.uint8)
    ctx._check(_raw_stereogram(ctx, od, mn, mx, case.out_w, case.out_h, case.amplitude,
                               X.stereo_noise(case.out_w, case.out_h), out))
    assert np.array_equal(out, want)


@pytest.mark.parametrize("name", ["96x40-257x3-a0.0625", "1026x3-70x200-a0.0625", "96x40-nan-513x2-a0.0625"])
def test_stereogram_with_the_range_on_the_device(name):
    """DepthMap::new -> output_stereogram chained on a tall map: me_depth_clamp_minmax_async, me_stereogram_dev_range"""
    ctx = _ctx()
    case = X.STEREO_BY_NAME[name]
    od, mn, mx = X.stereo_map(case.map)
    ddm = m.DeviceDepthMap(ctx, torch.from_numpy(od.copy()).cuda(), (case.out_w, case.out_h))
    noise = torch.from_numpy(np.array(X.stereo_noise(case.out_w, case.out_h))).cuda()
    got = ddm.stereogram(case.amplitude, noise)
    assert ddm.inverse_depth_range() == (mn, mx)
    assert np.array_equal(got.cpu().numpy(), X.stereo_oracle(name)[1])


@pytest.mark.parametrize("name", ["300x2-70x200-a0.0625", "96x40-257x3-a0.125"])
def test_stereogram_png_of_a_tall_map(tmp_path, name):
    from PIL import Image
    ctx = _ctx()
    case = X.STEREO_BY_NAME[name]
    od, _, _ = X.stereo_map(case.map)
    dm = m.DepthMap(ctx, od, (case.out_w, case.out_h))
    dm.output_stereogram_png(str(tmp_path / "s.png"), None, case.amplitude, X.stereo_noise(case.out_w, case.out_h))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "s.png")), X.stereo_oracle(name)[1])


def test_stereogram_refuses_a_row_wider_than_16384():
    ctx = _ctx()
    od, mn, mx = X.stereo_map("96x40")
    noise = np.zeros((1, 16385, 3), np.uint8)
    out = np.full((1, 16385, 3), 0xa5, np.uint8)
    assert _raw_stereogram(ctx, od, mn, mx, 16385, 1, 1.0 / 16.0, noise, out) == BAD_SHAPE
    assert "16384" in _last_error(ctx) and (out == 0xa5).all()
    assert ctx.status_flags() == 0


def test_stereogram_entries_refuse_a_wide_map(tmp_path):
    """cols > rows: the reference's sampler reads data[cols * y + x] past the end of the map and panics (the oracle's -1,
    tests/test_output_cases_cpu.py); all four entries return ME_ERR_BAD_SHAPE with a message that names the shape, before the
    kernel is launched, the caller's buffer written or the file created -- and the context goes on working."""
    ctx = _ctx()
    od, mn, mx = X.stereo_map("40x96")
    assert od.shape == (40, 96)
    out_w, out_h, amp = 64, 192, 1.0 / 16.0
    noise = X.stereo_noise(out_w, out_h)
    png, jpg = tmp_path / "wide.png", tmp_path / "wide.jpg"

    def refused(rc):
        msg = _last_error(ctx)
        return rc == BAD_SHAPE and "40x96" in msg and "rows >= cols" in msg

    # host pointers
    out = np.full((out_h, out_w, 3), 0xa5, np.uint8)
    assert refused(_raw_stereogram(ctx, od, mn, mx, out_w, out_h, amp, noise, out))
    assert (out == 0xa5).all()
    # device pointers, the range in device memory
    ddev = torch.from_numpy(od.copy()).cuda()
    ndev = torch.from_numpy(np.array(noise)).cuda()
    odev = torch.full((out_h, out_w, 3), 0xa5, dtype=torch.uint8, device="cuda")
    rdev = torch.tensor([mn, mx], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for o in (odev, out):
        assert refused(ctx.lib.me_stereogram_dev_range(ctx.handle, _vp(ddev), 40, 96, _vp(rdev), out_w, out_h, amp,
                                                       _vp(ndev), _vp(o)))
    assert refused(_raw_stereogram(ctx, ddev, mn, mx, out_w, out_h, amp, ndev, odev))
    ctx.synchronize()
    assert bool((odev == 0xa5).all()) and (out == 0xa5).all()
    assert np.array_equal(_bits(ddev), _bits(od))
    # the file entries
    for depth, nz in ((od, noise), (ddev, ndev)):
        assert refused(ctx.lib.me_output_stereogram_png(ctx.handle, _vp(depth), 40, 96, mn, mx, out_w, out_h, amp, _vp(nz),
                                                        str(png).encode()))
        assert refused(ctx.lib.me_output_stereogram_jpeg(ctx.handle, _vp(depth), 40, 96, mn, mx, out_w, out_h, amp, _vp(nz),
                                                         75, 2, str(jpg).encode()))
    assert not png.exists() and not jpg.exists() and os.listdir(tmp_path) == []
    # the Python mirror has no check of its own: the library's error comes through
    with pytest.raises(m.MatrixEyesError) as e:
        m.DepthMap(ctx, od, (out_w, out_h)).stereogram(None, amp, noise)
    assert e.value.code == BAD_SHAPE and "40x96" in e.value.message
    assert ctx.status_flags() == 0
    # the very next call on the context
    name = "96x40-257x3-a0.0625"
    case = X.STEREO_BY_NAME[name]
    tall, tmn, tmx = X.stereo_map(case.map)
    out = np.empty((case.out_h, case.out_w, 3), np.uint8)
    ctx._check(_raw_stereogram(ctx, tall, tmn, tmx, case.out_w, case.out_h, case.amplitude,
                               X.stereo_noise(case.out_w, case.out_h), out))
    assert np.array_equal(out, X.stereo_oracle(name)[1])
