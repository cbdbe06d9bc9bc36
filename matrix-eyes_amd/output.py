"""Host-side mirror of reference src/output.rs over the C ABI: DepthMap::new (output.rs:44-67),
output_image (:100-121), output_depth_map (:123-139), output_stereogram (:141-193),
output_mesh (:195-261)."""
import ctypes as C
import enum
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .depth_pro import (Context, _device_file, _in_ptr, noise_key, resolve_jpeg_encoder, resolve_jpeg_quality,
                        resolve_jpeg_subsampling, resolve_noise_source, resolve_png_encoder, resolve_resampler)


class VertexMode(enum.IntEnum):   # output.rs:33-38
    Plain = 0
    Color = 1
    Texture = 2


@dataclass
class ImageOutputFormat:           # output.rs:27-31
    kind: str = "depthmap"         # "depthmap" | "stereogram"
    resize_scale: Optional[float] = None
    amplitude: float = 1.0 / 16.0  # main.rs default --stereo-amplitude

    @staticmethod
    def DepthMap():
        return ImageOutputFormat("depthmap")

    @staticmethod
    def Stereogram(resize_scale: Optional[float], amplitude: float):
        return ImageOutputFormat("stereogram", resize_scale, amplitude)


def _f32_round(x: float) -> int:
    """f32::round (half away from zero, exact) of an f32 value, then `as u32` (saturating, NaN -> 0)."""
    x = np.float32(x)
    if not np.isfinite(x):
        return 0 if (np.isnan(x) or x < 0) else 4294967295
    t = np.trunc(x)
    if abs(x - t) >= np.float32(0.5):      # x - trunc(x) is exact in f32
        t += np.sign(x)
    if t <= 0:
        return 0
    return int(min(float(t), 4294967295.0))


def _noise_rng():
    """The stand-in for the reference's rand::rng(): seeded from the OS, or -- as the compiled CLI does -- from
    MATRIX_EYES_SEED, which makes a run repeatable (the reference is not)."""
    import os
    seed = os.environ.get("MATRIX_EYES_SEED")
    return np.random.default_rng(int(seed) if seed else None)


class DepthMap:
    def __init__(self, ctx: Context, inverse_depth, original_size):
        """DepthMap::new: clamp to [1/250, 1/0.1] (output.rs:51-57).  inverse_depth [rows, cols]."""
        self.ctx = ctx
        data = np.array(inverse_depth, dtype=np.float32, copy=True)
        if data.ndim != 2:
            raise L.MatrixEyesError(2, "DepthMap: inverse_depth must be 2-D")
        self.data_width, self.data_height = data.shape   # output.rs:52 (names as in the reference)
        mn, mx = C.c_float(), C.c_float()
        ctx._check(ctx.lib.me_depth_clamp_minmax(ctx.handle, C.c_void_p(data.ctypes.data), data.size,
                                                 C.byref(mn), C.byref(mx)))
        self.data = data
        self._range = (mn.value, mx.value)
        self.original_width, self.original_height = original_size

    def inverse_depth_range(self):   # output.rs:69-75
        return self._range

    # -- raster products (arrays; files below)
    def depth_map_rgb(self) -> np.ndarray:
        """output.rs:123-131 before the Lanczos resize -> u8 [data_width, data_height, 3]"""
        mn, mx = self._range
        out = np.empty(self.data.shape + (3,), np.uint8)
        self.ctx._check(self.ctx.lib.me_depthmap_rgb(self.ctx.handle, C.c_void_p(self.data.ctypes.data),
                                                     self.data.size, mn, mx, C.c_void_p(out.ctypes.data)))
        return out

    def stereogram_size(self, resize_scale: Optional[float]):
        if resize_scale is not None:   # output.rs:147-151, f32 arithmetic
            w = _f32_round(np.float32(self.original_width) * np.float32(resize_scale))
            h = _f32_round(np.float32(self.original_height) * np.float32(resize_scale))
            return w, h
        return self.original_width, self.original_height

    def _stereogram_noise(self, resize_scale, noise, noise_source=None, key=None):
        """(out_w, out_h, the noise's pointer or None, the key's buffer or None, a keepalive) of the stereogram methods;
        noise, noise_source and key as for `stereogram`.  Exactly one of the pointer and the key is set: the key with
        noise_source "device", which takes the keyed entries."""
        w, h = self.stereogram_size(resize_scale)
        if noise is None:
            source = resolve_noise_source(noise_source)
            if source == "legacy":
                noise = _noise_rng().integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            else:
                kbuf = (C.c_uint8 * 32).from_buffer_copy(noise_key(self.ctx.lib, key))
                if source == "device":
                    return w, h, None, kbuf, None
                noise = np.empty((h, w, 3), np.uint8)
                rc = self.ctx.lib.me_stereogram_noise_host(kbuf, w, h, C.c_void_p(noise.ctypes.data))
                if rc != L.ME_OK:
                    L.check(self.ctx.lib, None, rc)
        pn, keep = _in_ptr(noise, np.uint8)
        if tuple(noise.shape) != (h, w, 3):
            raise L.MatrixEyesError(2, f"noise must be [{h},{w},3]")
        return w, h, pn, None, keep

    def stereogram(self, resize_scale: Optional[float], amplitude: float, noise=None, noise_source=None, key=None) -> np.ndarray:
        """output.rs:141-193 -> u8 [out_h, out_w, 3].  noise u8 [out_h, out_w, 3] stands in for the
        reference's rand::rng() stream (row by row, pixel by pixel).  When omitted it comes from noise_source
        (depth_pro.resolve_noise_source): "legacy" draws it from numpy seeded with MATRIX_EYES_SEED or the OS; "host" and
        "device" make the keyed noise of `key` (32 bytes; None: depth_pro.noise_key) on the CPU or on the GPU."""
        w, h, pn, kbuf, keep = self._stereogram_noise(resize_scale, noise, noise_source, key)
        mn, mx = self._range
        out = np.empty((h, w, 3), np.uint8)
        entry = self.ctx.lib.me_stereogram if kbuf is None else self.ctx.lib.me_stereogram_keyed
        self.ctx._check(entry(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, mn, mx,
            w, h, amplitude, pn if kbuf is None else kbuf, C.c_void_p(out.ctypes.data)))
        return out

    def mesh_index(self, want_faces=True):
        """IndexedMesh::new + remap_face (output.rs:264-363) -> (vertex_index [n], nverts, faces)"""
        w, h = self.data_width, self.data_height
        vi = np.empty((w * h,), np.int32)
        faces = np.empty((2 * (w - 1) * (h - 1), 3), np.int32) if want_faces else None
        nv, nf = C.c_int64(), C.c_int64()
        self.ctx._check(self.ctx.lib.me_mesh_index(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), w, h, C.c_void_p(vi.ctypes.data),
            C.byref(nv), C.byref(nf), C.c_void_p(faces.ctypes.data) if want_faces else None))
        return vi, nv.value, (faces[:nf.value] if want_faces else nf.value)

    def mesh_vertices(self, vertex_index, nverts):
        """output.rs:228-249 -> (uv [n,2], xyz [n,3]) in vertex-id order"""
        uv = np.empty((nverts, 2), np.float32)
        xyz = np.empty((nverts, 3), np.float32)
        pv, keep = _in_ptr(vertex_index, np.int32)
        self.ctx._check(self.ctx.lib.me_mesh_vertices(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, pv,
            nverts, self.original_width, self.original_height, C.c_void_p(uv.ctypes.data),
            C.c_void_p(xyz.ctypes.data)))
        return uv, xyz

    # -- files
    def depth_map_rgb_resized(self) -> np.ndarray:
        """output.rs:123-137 up to the save, on the GPU: the colour map, then the `image` crate's Lanczos3 resize to
        the original size -> u8 [original_height, original_width, 3]"""
        mn, mx = self._range
        out = np.empty((self.original_height, self.original_width, 3), np.uint8)
        self.ctx._check(self.ctx.lib.me_depthmap_rgb_resized(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, mn, mx, None,
            self.original_width, self.original_height, C.c_void_p(out.ctypes.data)))
        return out

    def output_depth_map_png(self, destination_path: str):
        """output.rs:123-139 whole, on the GPU (me_output_depth_map_png): colour map, Lanczos3 resize, PNG file"""
        mn, mx = self._range
        self.ctx._check(self.ctx.lib.me_output_depth_map_png(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, mn, mx, None,
            self.original_width, self.original_height, str(destination_path).encode()))

    def output_stereogram_png(self, destination_path: str, resize_scale: Optional[float], amplitude: float, noise=None,
                              noise_source=None, key=None):
        """output.rs:141-193 whole, on the GPU (me_output_stereogram_png, or its _keyed form); noise, noise_source and key
        as for `stereogram`"""
        w, h, pn, kbuf, keep = self._stereogram_noise(resize_scale, noise, noise_source, key)
        mn, mx = self._range
        entry = self.ctx.lib.me_output_stereogram_png if kbuf is None else self.ctx.lib.me_output_stereogram_png_keyed
        self.ctx._check(entry(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, mn, mx,
            w, h, amplitude, pn if kbuf is None else kbuf, str(destination_path).encode()))

    def output_depth_map_jpeg(self, destination_path: str, quality: int = 75, subsampling: int = 2):
        """output.rs:123-139 whole, on the GPU (me_output_depth_map_jpeg): colour map, Lanczos3 resize, JPEG file"""
        mn, mx = self._range
        self.ctx._check(self.ctx.lib.me_output_depth_map_jpeg(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, mn, mx, None,
            self.original_width, self.original_height, int(quality), int(subsampling), str(destination_path).encode()))

    def output_stereogram_jpeg(self, destination_path: str, resize_scale: Optional[float], amplitude: float, noise=None,
                               quality: int = 75, subsampling: int = 2, noise_source=None, key=None):
        """output.rs:141-193 whole, on the GPU (me_output_stereogram_jpeg, or its _keyed form); noise, noise_source and key
        as for `stereogram`"""
        w, h, pn, kbuf, keep = self._stereogram_noise(resize_scale, noise, noise_source, key)
        mn, mx = self._range
        entry = self.ctx.lib.me_output_stereogram_jpeg if kbuf is None else self.ctx.lib.me_output_stereogram_jpeg_keyed
        self.ctx._check(entry(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, mn, mx,
            w, h, amplitude, pn if kbuf is None else kbuf, int(quality), int(subsampling), str(destination_path).encode()))

    def output_image(self, destination_path: str, source_path: str, image_format: ImageOutputFormat,
                     vertex_mode: VertexMode, noise=None, resampler=None, png_encoder=None, jpeg_encoder=None,
                     jpeg_quality=None, jpeg_subsampling=None, noise_source=None):
        """output.rs:100-121: dispatch on the destination suffix.  noise_source: depth_pro.resolve_noise_source, for a
        stereogram without `noise`; resampler: depth_pro.resolve_resampler;
        png_encoder: depth_pro.resolve_png_encoder; jpeg_encoder, jpeg_quality, jpeg_subsampling:
        depth_pro.resolve_jpeg_encoder / _quality / _subsampling (they act on a ".jpg" / ".jpeg" destination only)."""
        resampler = resolve_resampler(resampler)
        png_encoder = resolve_png_encoder(png_encoder)
        jpeg_encoder = resolve_jpeg_encoder(jpeg_encoder)
        noise_source = resolve_noise_source(noise_source)
        low = destination_path.lower()
        if low.endswith((".ply", ".obj", ".glb")):   # (.glb: glTF 2.0 binary, beyond the reference's two)
            return self.output_mesh(destination_path, source_path, vertex_mode, resampler=resampler)
        from PIL import Image
        jpeg = low.endswith(".jpg") or low.endswith(".jpeg")
        save_args, jpeg_args = {}, ()
        if jpeg:
            # both paths are defined by the same numbers: Pillow's own defaults, spelled out
            jpeg_args = quality, subsampling = resolve_jpeg_quality(jpeg_quality), resolve_jpeg_subsampling(jpeg_subsampling)
            save_args = {"format": "JPEG", "quality": quality, "subsampling": subsampling, "optimize": False}
        if (jpeg_encoder == "device") if jpeg else (png_encoder == "device" and low.endswith(".png")):
            stereogram, depth_map, picture = ((self.output_stereogram_jpeg, self.output_depth_map_jpeg, self.ctx.output_jpeg) if jpeg
                                              else (self.output_stereogram_png, self.output_depth_map_png, self.ctx.output_png))
            native = self.original_width == self.original_height == self.data_width == self.data_height
            if image_format.kind != "depthmap":
                return stereogram(destination_path, image_format.resize_scale, image_format.amplitude, noise, *jpeg_args,
                                  noise_source=noise_source)
            if resampler == "device" or native:   # (the resize is the identity at the native size)
                return depth_map(destination_path, *jpeg_args)
            img = Image.fromarray(self.depth_map_rgb()).resize((self.original_width, self.original_height), Image.LANCZOS)
            return picture(np.asarray(img, dtype=np.uint8), destination_path, *jpeg_args)
        if image_format.kind == "depthmap" and resampler == "device":
            Image.fromarray(self.depth_map_rgb_resized()).save(destination_path, **save_args)
        elif image_format.kind == "depthmap":
            img = Image.fromarray(self.depth_map_rgb())
            size = (self.original_width, self.original_height)
            if img.size != size:   # output.rs:133-137 (identity at the native size)
                img = img.resize(size, Image.LANCZOS)
            img.save(destination_path, **save_args)
        else:
            Image.fromarray(self.stereogram(image_format.resize_scale, image_format.amplitude, noise,
                                            noise_source=noise_source)).save(destination_path, **save_args)

    def output_mesh(self, destination_path: str, source_path: str, vertex_mode: VertexMode, resampler=None):
        """output.rs:195-261 with ObjWriter / PlyWriter; a ".glb" destination is a glTF 2.0 binary mesh (mesh_glb_bytes)."""
        resampler = resolve_resampler(resampler)
        colors = None
        if vertex_mode == VertexMode.Color:   # output.rs:206-218
            from PIL import Image
            img = Image.open(source_path).convert("RGB")
            if resampler == "device":
                colors = self.ctx.resize_lanczos3(np.asarray(img, dtype=np.uint8), (self.data_width, self.data_height))
            else:
                colors = np.ascontiguousarray(np.asarray(
                    img.resize((self.data_width, self.data_height), Image.LANCZOS), dtype=np.uint8))
        self.ctx._check(self.ctx.lib.me_output_mesh(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height,
            self.original_width, self.original_height, destination_path.encode(), source_path.encode(),
            int(vertex_mode), C.c_void_p(colors.ctypes.data) if colors is not None else None))

    def mesh_ply_bytes(self, vertex_mode: VertexMode = VertexMode.Plain, colors=None) -> bytes:
        """The PLY file output_mesh(".ply") writes, as `bytes` (me_mesh_ply_bytes: the records packed on the GPU).
        colors: u8 [data_height, data_width, 3] (the source resized to the depth map) or None, read in VertexMode.Color only."""
        if colors is not None:
            colors = np.ascontiguousarray(colors, dtype=np.uint8)
        ptr, n = C.c_void_p(), C.c_int64()
        self.ctx._check(self.ctx.lib.me_mesh_ply_bytes(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, self.original_width,
            self.original_height, int(vertex_mode), C.c_void_p(colors.ctypes.data) if colors is not None else None,
            C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, self.data)

    def mesh_glb_bytes(self, source_path: str = "", vertex_mode: VertexMode = VertexMode.Plain, colors=None) -> bytes:
        """The glTF 2.0 binary file output_mesh(".glb") writes, as `bytes` (me_mesh_glb_bytes: the sections packed on the
        GPU).  source_path: the picture a VertexMode.Texture material names; colors: as for mesh_ply_bytes."""
        if colors is not None:
            colors = np.ascontiguousarray(colors, dtype=np.uint8)
        ptr, n = C.c_void_p(), C.c_int64()
        self.ctx._check(self.ctx.lib.me_mesh_glb_bytes(
            self.ctx.handle, C.c_void_p(self.data.ctypes.data), self.data_width, self.data_height, self.original_width,
            self.original_height, str(source_path).encode(), int(vertex_mode),
            C.c_void_p(colors.ctypes.data) if colors is not None else None, C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, self.data)


class DeviceDepthMap:
    """DepthMap::new -> output_image chained on the GPU (BASELINE configs[4]: depth -> stereogram / depth map
    without the host round trips of the reference's readback, output.rs:44-67).  `inverse_depth` is a CUDA f32
    tensor [rows, cols] (e.g. the `out=` tensor of Context.extract_depth); it is clamped IN PLACE on the context's
    stream and its range stays in device memory for the raster kernels queued behind it."""

    def __init__(self, ctx: Context, inverse_depth, original_size):
        import torch
        if not (inverse_depth.is_cuda and inverse_depth.dtype == torch.float32 and inverse_depth.dim() == 2
                and inverse_depth.is_contiguous()):
            raise L.MatrixEyesError(2, "DeviceDepthMap: a contiguous CUDA f32 [rows, cols] tensor is required")
        self.ctx, self.data = ctx, inverse_depth
        self.data_width, self.data_height = inverse_depth.shape
        self.original_width, self.original_height = original_size
        self.range_dev = torch.empty(2, dtype=torch.float32, device=inverse_depth.device)
        ctx._check(ctx.lib.me_depth_clamp_minmax_async(ctx.handle, C.c_void_p(inverse_depth.data_ptr()),
                                                       inverse_depth.numel(), C.c_void_p(self.range_dev.data_ptr())))

    def inverse_depth_range(self):
        self.ctx.synchronize()
        mn, mx = self.range_dev.tolist()
        return mn, mx

    def depth_map_rgb(self, out=None):
        import torch
        if out is None:
            out = torch.empty(self.data.shape + (3,), dtype=torch.uint8, device=self.data.device)
        self.ctx._check(self.ctx.lib.me_depthmap_rgb_dev_range(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data.numel(), C.c_void_p(self.range_dev.data_ptr()),
            C.c_void_p(out.data_ptr())))
        return out

    def depth_map_rgb_resized(self, out=None):
        """output.rs:123-137 up to the save, chained on the stream: colour map, then the Lanczos3 resize to the original
        size -> CUDA u8 [original_height, original_width, 3]"""
        import torch
        shape = (self.original_height, self.original_width, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.data.device)
        self.ctx._check(self.ctx.lib.me_depthmap_rgb_resized(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data_width, self.data_height, 0.0, 0.0,
            C.c_void_p(self.range_dev.data_ptr()), self.original_width, self.original_height, C.c_void_p(out.data_ptr())))
        return out

    def output_mesh(self, destination_path: str, source_path: str, vertex_mode: VertexMode = VertexMode.Texture,
                    colors=None):
        """output.rs:195-261 from the device-resident depth: mesh indexing, vertex coordinates and (OBJ) the text
        itself are produced on the GPU; only the finished file bytes cross to the host."""
        self.ctx._check(self.ctx.lib.me_output_mesh(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data_width, self.data_height,
            self.original_width, self.original_height, destination_path.encode(), source_path.encode(),
            int(vertex_mode), C.c_void_p(colors.data_ptr()) if colors is not None else None))

    def obj_text(self, stem: str = "mesh", vertex_mode: VertexMode = VertexMode.Texture, colors=None):
        """The OBJ file's bytes as a CUDA uint8 tensor (me_mesh_obj_text: the text formatted on the GPU; a copy of the
        context-owned buffer)."""
        ptr, n = C.c_void_p(), C.c_int64()
        self.ctx._check(self.ctx.lib.me_mesh_obj_text(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data_width, self.data_height, self.original_width,
            self.original_height, stem.encode(), int(vertex_mode),
            C.c_void_p(colors.data_ptr()) if colors is not None else None, C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, self.data)

    def mesh_ply_bytes(self, vertex_mode: VertexMode = VertexMode.Plain, colors=None):
        """The PLY file's bytes as a CUDA uint8 tensor (me_mesh_ply_bytes: the records packed on the GPU; a copy of the
        context-owned buffer).  colors: CUDA u8 [rows, cols, 3] or None, read in VertexMode.Color only."""
        ptr, n = C.c_void_p(), C.c_int64()
        self.ctx._check(self.ctx.lib.me_mesh_ply_bytes(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data_width, self.data_height, self.original_width,
            self.original_height, int(vertex_mode), C.c_void_p(colors.data_ptr()) if colors is not None else None,
            C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, self.data)

    def mesh_glb_bytes(self, source_path: str = "", vertex_mode: VertexMode = VertexMode.Plain, colors=None):
        """The glTF 2.0 binary file's bytes as a CUDA uint8 tensor (me_mesh_glb_bytes; a copy of the context-owned
        buffer).  colors: CUDA u8 [rows, cols, 3] or None, read in VertexMode.Color only."""
        ptr, n = C.c_void_p(), C.c_int64()
        self.ctx._check(self.ctx.lib.me_mesh_glb_bytes(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data_width, self.data_height, self.original_width,
            self.original_height, str(source_path).encode(), int(vertex_mode),
            C.c_void_p(colors.data_ptr()) if colors is not None else None, C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, self.data)

    def stereogram(self, amplitude: float, noise=None, out=None, key=None, size=None):
        """noise: CUDA u8 [out_h, out_w, 3]; or key=: the 32 bytes of the keyed noise, made on the
        device for a picture of size = (out_w, out_h) (default: the original size) -- me_stereogram_keyed_dev_range"""
        import torch
        if (noise is None) == (key is None):
            raise L.MatrixEyesError(1, "DeviceDepthMap.stereogram: pass either noise or key")
        if key is None:
            h, w = noise.shape[0], noise.shape[1]
            entry, source = self.ctx.lib.me_stereogram_dev_range, C.c_void_p(noise.data_ptr())
        else:
            w, h = size if size is not None else (self.original_width, self.original_height)
            entry = self.ctx.lib.me_stereogram_keyed_dev_range
            source = (C.c_uint8 * 32).from_buffer_copy(noise_key(self.ctx.lib, key))
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=self.data.device)
        self.ctx._check(entry(
            self.ctx.handle, C.c_void_p(self.data.data_ptr()), self.data_width, self.data_height,
            C.c_void_p(self.range_dev.data_ptr()), w, h, amplitude, source, C.c_void_p(out.data_ptr())))
        return out
