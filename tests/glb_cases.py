"""Shared by tests/test_glb_cpu.py and tests/test_gpu_glb.py: an independent restatement of the .glb file the mesh back end
writes (numpy, struct, json and the oracle's number text; not a port of csrc/glb_format.h) and a structural checker of
such a file.  No glTF library is installed where these tests run, so check_glb is the validator: it holds the container,
the chunk padding, the alignments, the views, the accessors and the index range to the glTF 2.0 rules the format uses."""
import json
import struct

import numpy as np

from oracle import output_oracle as OO

COUNTS = (1, 3, 4, 5, 255, 256, 257, 1000)      # V and F around a 16-byte unit (4 vertices) and a workgroup (256 units); 0 is the empty asset
MODES = ("plain", "color", "texture")
GENERATOR = "Matrix Eyes 3D surface"


class Refused(ValueError):
    """the mesh has no .glb file: a position bound that is not finite, or 2^32 bytes and more"""


def _up(n, m):
    return -(-n // m) * m


def _bound_text(column, largest):
    """min or max of an f32 column as the text of an OBJ "v" number; among zeros of both signs -0 is the smaller"""
    if not np.isfinite(column).all():
        raise Refused("bound not finite")
    v = column.max() if largest else column.min()
    if v == 0:
        zeros = column[column == 0]
        negative = np.signbit(zeros).all() if largest else np.signbit(zeros).any()
        v = np.float32(-0.0) if negative else np.float32(0.0)
    return OO.rust_display_f64(float(v))


def escape(source):
    """JSON string body: `"`, `\\` and control bytes as \\u00xx; everything else, UTF-8 included, verbatim"""
    out = bytearray()
    for b in source.encode() if isinstance(source, str) else bytes(source):
        if b in (0x22, 0x5C):
            out += b"\\" + bytes([b])
        elif b < 0x20:
            out += b"\\u%04x" % b
        else:
            out.append(b)
    return bytes(out)


def written_positions(xyz):
    p = np.array(xyz, np.float32).reshape(-1, 3)
    p[:, 1:] = -p[:, 1:]
    return p


def glb_bytes(xyz, uv, faces, mode, colors=None, source=""):
    """the whole file: xyz [V,3] f32 and uv [V,2] f32 of mesh_vertices, faces [F,3], mode 'plain' | 'color' | 'texture',
    colors u8 [V,3] per vertex id or None, source the picture's path"""
    pos = written_positions(xyz)
    nv = len(pos)
    asset = {"asset": {"version": "2.0", "generator": GENERATOR}, "scene": 0}
    if nv == 0:
        asset["scenes"] = [{"nodes": []}]
        text = json.dumps(asset, separators=(",", ":")).encode()
        text += b" " * ((4 - len(text)) % 16)
        return b"glTF" + struct.pack("<III", 2, 20 + len(text), len(text)) + b"JSON" + text
    idx = np.asarray(faces).reshape(-1, 3).astype("<u4")
    sections = [("POSITION", pos.astype("<f4").tobytes(), 34962,
                 {"componentType": 5126, "count": nv, "type": "VEC3", "min": ["@min%d@" % c for c in range(3)],
                  "max": ["@max%d@" % c for c in range(3)]})]
    if mode == "color" and colors is not None:
        rgba = np.full((nv, 4), 255, np.uint8)
        rgba[:, :3] = np.asarray(colors, np.uint8).reshape(-1, 3)
        sections.append(("COLOR_0", rgba.tobytes(), 34962, {"componentType": 5121, "normalized": True, "count": nv, "type": "VEC4"}))
    if mode == "texture":
        sections.append(("TEXCOORD_0", np.asarray(uv, np.float32).reshape(-1, 2).astype("<f4").tobytes(), 34962,
                         {"componentType": 5126, "count": nv, "type": "VEC2"}))
    sections.append((None, idx.tobytes(), 34963, {"componentType": 5125, "count": idx.size, "type": "SCALAR"}))
    binary, views, accessors, attributes = bytearray(), [], [], {}
    for k, (name, data, target, accessor) in enumerate(sections):
        binary += bytes(_up(len(binary), 16) - len(binary))
        views.append({"buffer": 0, "byteOffset": len(binary), "byteLength": len(data), "target": target})
        accessors.append({"bufferView": k, **accessor})
        if name:
            attributes[name] = k
        binary += data
    binary += bytes(_up(len(binary), 4) - len(binary))
    material = {"pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 1}, "doubleSided": True}
    asset.update({"scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
                  "meshes": [{"primitives": [{"attributes": attributes, "indices": len(sections) - 1, "material": 0, "mode": 4}]}],
                  "materials": [material]})
    if mode == "texture":
        material["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 0}
        asset.update({"textures": [{"source": 0}], "images": [{"uri": "@uri@"}]})
    asset.update({"buffers": [{"byteLength": len(binary)}], "bufferViews": views, "accessors": accessors})
    text = json.dumps(asset, separators=(",", ":")).encode()
    for c in range(3):
        text = text.replace(b'"@min%d@"' % c, _bound_text(pos[:, c], False).encode())
        text = text.replace(b'"@max%d@"' % c, _bound_text(pos[:, c], True).encode())
    text = text.replace(b"@uri@", escape(source))
    text += b" " * ((4 - len(text)) % 16)
    total = 12 + 8 + len(text) + 8 + len(binary)
    if total >= 2 ** 32:
        raise Refused("too large")
    return (b"glTF" + struct.pack("<III", 2, total, len(text)) + b"JSON" + text + struct.pack("<I", len(binary)) + b"BIN\0" +
            bytes(binary))


_TOP = ["asset", "scene", "scenes", "nodes", "meshes", "materials", "textures", "images", "buffers", "bufferViews", "accessors"]


def check_glb(data, referenced=True):
    """Structural checks of a file of this writer -> {"json", "positions", "colors", "uvs", "indices"} (arrays, or None).
    referenced=False: the test's faces are random and need not use every vertex."""
    data = bytes(data)
    magic, version, total, jlen, jtype = struct.unpack_from("<4sIII4s", data, 0)
    assert (magic, version, total, jtype) == (b"glTF", 2, len(data), b"JSON")
    assert jlen % 4 == 0 and jlen % 16 == 4, jlen
    text = data[20:20 + jlen]
    body = text.rstrip(b" ")
    assert body.startswith(b"{") and body.endswith(b"}")
    in_string, escaped = False, False
    for b in body:                                  # no whitespace outside strings
        if in_string:
            in_string, escaped = not (b == 0x22 and not escaped), b == 0x5C and not escaped
        else:
            assert b not in b" \t\r\n"
            in_string = b == 0x22
    assert not in_string
    j = json.loads(body.decode())
    assert list(j["asset"]) == ["version", "generator"] and j["asset"] == {"version": "2.0", "generator": GENERATOR}
    assert list(j) == [k for k in _TOP if k in j] and j["scene"] == 0
    out = {"json": j, "positions": None, "colors": None, "uvs": None, "indices": None}
    if "meshes" not in j:
        assert list(j) == ["asset", "scene", "scenes"] and j["scenes"] == [{"nodes": []}] and len(data) == 20 + jlen
        return out
    blen, btype = struct.unpack_from("<I4s", data, 20 + jlen)
    assert btype == b"BIN\0" and blen % 4 == 0 and 28 + jlen + blen == len(data) and (28 + jlen) % 16 == 0
    binary = data[28 + jlen:]
    assert j["scenes"] == [{"nodes": [0]}] and j["nodes"] == [{"mesh": 0}] and j["buffers"] == [{"byteLength": blen}]
    (prim,), (material,) = j["meshes"][0]["primitives"], j["materials"]
    assert list(prim) == ["attributes", "indices", "material", "mode"] and prim["material"] == 0 and prim["mode"] == 4
    assert list(material) == ["pbrMetallicRoughness", "doubleSided"] and material["doubleSided"] is True
    pbr = material["pbrMetallicRoughness"]
    textured = "textures" in j
    assert list(pbr) == ["metallicFactor", "roughnessFactor"] + (["baseColorTexture"] if textured else [])
    assert pbr["metallicFactor"] == 0 and pbr["roughnessFactor"] == 1
    if textured:
        assert pbr["baseColorTexture"] == {"index": 0} and j["textures"] == [{"source": 0}] and list(j["images"][0]) == ["uri"]
        assert "TEXCOORD_0" in prim["attributes"]
    else:
        assert "images" not in j
    views, accessors = j["bufferViews"], j["accessors"]
    assert len(views) == len(accessors) == prim["indices"] + 1 == len(prim["attributes"]) + 1
    assert list(prim["attributes"]) == ["POSITION"] + [k for k in ("COLOR_0", "TEXCOORD_0") if k in prim["attributes"]]
    assert list(prim["attributes"].values()) == list(range(len(prim["attributes"])))
    covered = np.zeros(blen, bool)
    for k, (v, a) in enumerate(zip(views, accessors)):
        assert list(v) == ["buffer", "byteOffset", "byteLength", "target"] and v["buffer"] == 0 and a["bufferView"] == k
        assert v["byteOffset"] % 16 == 0 and v["byteLength"] > 0 and v["byteOffset"] + v["byteLength"] <= blen
        assert v["target"] == (34963 if k == prim["indices"] else 34962)
        assert not covered[v["byteOffset"]:v["byteOffset"] + v["byteLength"]].any()
        covered[v["byteOffset"]:v["byteOffset"] + v["byteLength"]] = True
    assert not np.frombuffer(binary, np.uint8)[~covered].any()           # gaps and tail are zeros
    assert blen == _up(views[-1]["byteOffset"] + views[-1]["byteLength"], 4)

    def array(k, dtype, width):
        v, a = views[k], accessors[k]
        assert v["byteLength"] == a["count"] * width * np.dtype(dtype).itemsize
        return np.frombuffer(binary, dtype, a["count"] * width, v["byteOffset"]).reshape(-1, width)

    a0 = accessors[0]
    assert list(a0) == ["bufferView", "componentType", "count", "type", "min", "max"] and (a0["componentType"], a0["type"]) == (5126, "VEC3")
    pos = out["positions"] = array(0, "<f4", 3)
    nv = len(pos)
    assert nv > 0 and np.isfinite(pos).all()
    # the bounds' text reads back (as f64, then narrowed: they are f32 values) to the data's bounds, exactly
    for key, bound in (("min", pos.min(0)), ("max", pos.max(0))):
        stated = np.array([float(v) for v in a0[key]], np.float64)               # (json reads "3" as an int of any size)
        assert len(stated) == 3 and np.array_equal(stated, bound.astype(np.float64)) and np.array_equal(stated.astype(np.float32), bound)
    if "COLOR_0" in prim["attributes"]:
        a1 = accessors[1]
        assert list(a1) == ["bufferView", "componentType", "normalized", "count", "type"]
        assert (a1["componentType"], a1["normalized"], a1["count"], a1["type"]) == (5121, True, nv, "VEC4")
        out["colors"] = array(1, np.uint8, 4)
        assert (out["colors"][:, 3] == 255).all()
    if "TEXCOORD_0" in prim["attributes"]:
        a1 = accessors[1]
        assert list(a1) == ["bufferView", "componentType", "count", "type"] and (a1["componentType"], a1["count"], a1["type"]) == (5126, nv, "VEC2")
        out["uvs"] = array(1, "<f4", 2)
    ai = accessors[-1]
    assert list(ai) == ["bufferView", "componentType", "count", "type"] and (ai["componentType"], ai["type"]) == (5125, "SCALAR")
    assert ai["count"] % 3 == 0 and ai["count"] > 0
    idx = out["indices"] = array(len(views) - 1, "<u4", 1).reshape(-1, 3)
    assert int(idx.max()) < nv
    if referenced:
        assert len(np.unique(idx)) == nv
    return out


def random_mesh(nverts, nfaces, seed):
    """(xyz [V,3], uv [V,2], faces [F,3] with ids < V that use every vertex when 3F >= V, rgb [V,3]): finite coordinates of
    many magnitudes and both signs, some zeros of both signs"""
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((nverts, 3)) * np.exp(rng.uniform(-20, 20, (nverts, 3)))).astype(np.float32)
    xyz[rng.random((nverts, 3)) < 0.05] = 0.0
    xyz[rng.random((nverts, 3)) < 0.05] = -0.0
    uv = rng.uniform(0, 1, (nverts, 2)).astype(np.float32)
    ids = rng.integers(0, max(nverts, 1), size=3 * nfaces, dtype=np.int64)
    if 3 * nfaces >= nverts:
        ids[rng.permutation(3 * nfaces)[:nverts]] = np.arange(nverts)
    rgb = rng.integers(0, 256, size=(nverts, 3), dtype=np.uint8)
    return xyz, uv, ids.astype(np.int32).reshape(-1, 3), rgb
