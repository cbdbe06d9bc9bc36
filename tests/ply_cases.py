"""Shared by tests/test_ply_cpu.py and tests/test_gpu_ply.py: a vectorised restatement of oracle.output_oracle.ply_bytes
(a Python loop, too slow for a 1536 x 1536 mesh) and the record-count sweep of the packing tests."""
import numpy as np

from oracle import output_oracle as OO

THREADS = 256                                   # me_ply::kThreads: records of one workgroup
COUNTS = (0, 1, 255, 256, 257, 1000)            # around one workgroup's span, and several workgroups
VERTEX_BYTES, COLOR_BYTES, FACE_BYTES = 24, 3, 13


def ply_header(nverts, nfaces, vertex_mode):
    head = ["ply", "format binary_big_endian 1.0", "comment Matrix Eyes 3D surface",
            f"element vertex {nverts}", "property double x", "property double y", "property double z"]
    if vertex_mode == "color":
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {nfaces}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(head) + "\n").encode()


def ply_body_fast(xyz, faces, colors=None):
    """the records of ply_bytes behind the header: x, -y, -z (negated in f32, then widened) as big-endian f64 [+ r g b];
    3 and three big-endian u32 per face"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    v = xyz.copy()
    v[:, 1:] = -v[:, 1:]
    vrec = np.empty((len(v), VERTEX_BYTES + (COLOR_BYTES if colors is not None else 0)), np.uint8)
    vrec[:, :VERTEX_BYTES] = np.ascontiguousarray(v.astype(">f8")).view(np.uint8).reshape(len(v), VERTEX_BYTES)
    if colors is not None:
        vrec[:, VERTEX_BYTES:] = np.asarray(colors, np.uint8).reshape(-1, 3)
    frec = np.empty((len(faces), FACE_BYTES), np.uint8)
    frec[:, 0] = 3
    frec[:, 1:] = np.ascontiguousarray(faces.astype(">u4")).view(np.uint8).reshape(len(faces), 12)
    return vrec.tobytes() + frec.tobytes()


def ply_bytes_fast(xyz, faces, vertex_mode, colors=None):
    use = colors if vertex_mode == "color" else None
    return ply_header(len(np.asarray(xyz).reshape(-1, 3)), len(np.asarray(faces).reshape(-1, 3)), vertex_mode) + \
        ply_body_fast(xyz, faces, use)


def random_mesh(nverts, nfaces, seed):
    """(xyz f32 [nverts,3], faces i32 [nfaces,3], rgb u8 [nverts,3]): coordinates of every magnitude and sign, ids up to
    2^31 - 1 (the packing does not look them up)"""
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((nverts, 3)) * np.exp(rng.uniform(-20, 20, (nverts, 3)))).astype(np.float32)
    faces = rng.integers(0, 2 ** 31, size=(nfaces, 3), dtype=np.int64).astype(np.int32)
    rgb = rng.integers(0, 256, size=(nverts, 3), dtype=np.uint8)
    return xyz, faces, rgb


def edge_vertices():
    """0.0, -0.0, an f32 subnormal, +-inf and +-FLT_MAX in each coordinate"""
    sub = np.array([1], np.uint32).view(np.float32)[0]          # 2^-149
    fmax = np.finfo(np.float32).max
    vals = np.array([0.0, -0.0, sub, -sub, np.inf, -np.inf, fmax, -fmax, np.finfo(np.float32).tiny, 1.0], np.float32)
    grid = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(grid)                           # 1000 vertices: every value in every coordinate


def check_restatement():
    """ply_bytes_fast is ply_bytes on small cases: plain, colour, colour without an array, texture; the edge values"""
    for nv, nf, seed in ((0, 0, 1), (1, 0, 2), (7, 5, 3), (257, 300, 4)):
        xyz, faces, rgb = random_mesh(nv, nf, seed)
        faces = faces % max(nv, 1)
        for mode, colors in (("plain", None), ("color", rgb), ("color", None), ("texture", None), ("plain", rgb)):
            assert ply_bytes_fast(xyz, faces, mode, colors) == OO.ply_bytes(xyz, faces, mode, colors), (nv, nf, mode)
    e = edge_vertices()[::7]
    with np.errstate(all="ignore"):
        assert ply_bytes_fast(e, np.zeros((0, 3), np.int32), "plain") == OO.ply_bytes(e, np.zeros((0, 3), np.int32), "plain")
