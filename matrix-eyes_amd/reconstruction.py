"""Host-side mirror of reference src/reconstruction.rs: image front end and the
top-level `extract_depth`.  File decoding and EXIF are Pillow's (the reference uses the `image` and
`kamadak-exif` crates); the Lanczos resampling is Pillow's too by default, or the library's
(resampler="device": the `image` crate's bytes); at the native 1536x1536 size the resize is the identity.
The u8 -> float normalisation and HWC -> CHW (reconstruction.rs:114-124) run on the GPU
(`me_extract_depth_u8`)."""
import math
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .depth_pro import IMG_SIZE, DepthProModelLoader, resolve_jpeg_decoder, resolve_jpeg_entropy, resolve_png_decoder, resolve_resampler
from .output import DepthMap, ImageOutputFormat, VertexMode

_EXIF_IFD = 0x8769
_FOCAL_LENGTH_35MM = 0xA405   # exif::Tag::FocalLengthIn35mmFilm (reconstruction.rs:136-137)


class ReconstructionError(RuntimeError):   # reconstruction.rs:240-249
    pass


@dataclass
class SourceImage:                          # reconstruction.rs:74-81
    rgb8: np.ndarray                        # u8 [IMG_SIZE, IMG_SIZE, 3]
    original_size: Tuple[int, int]          # (width, height) after orientation
    focal_length_35mm: Optional[float]

    @staticmethod
    def load(path: str, focal_length_35mm: Optional[float] = None, size: int = IMG_SIZE, resampler=None,
             ctx=None, jpeg_decoder=None, jpeg_entropy=None, png_decoder=None) -> "SourceImage":
        """reconstruction.rs:87-131: decode, EXIF focal length, orientation, Lanczos3 to size x size.
        resampler: depth_pro.resolve_resampler; "device" resizes on `ctx` (a Context, or a callable that returns one
        and is only called once the file has been decoded).  jpeg_decoder: depth_pro.resolve_jpeg_decoder; "device"
        decodes a .jpg / .jpeg source on `ctx` (Pillow still reads the EXIF block), chained with the resize when the
        resampler is "device" too; jpeg_entropy: depth_pro.resolve_jpeg_entropy, where that decoder runs the Huffman
        decoding.  png_decoder: depth_pro.resolve_png_decoder; "device" does the same for a .png source
        (me_png_decode_rgb8 / me_png_decode_resized_rgb8; Pillow reads the eXIf chunk)."""
        from PIL import Image, ImageOps
        resampler = resolve_resampler(resampler)
        jpeg_entropy = resolve_jpeg_entropy(jpeg_entropy)
        if resolve_jpeg_decoder(jpeg_decoder) == "device" and path.lower().endswith((".jpg", ".jpeg")):
            return SourceImage._load_on_device("jpeg", path, focal_length_35mm, size, resampler, ctx, jpeg_entropy)
        if resolve_png_decoder(png_decoder) == "device" and path.lower().endswith(".png"):
            return SourceImage._load_on_device("png", path, focal_length_35mm, size, resampler, ctx)
        try:
            img = Image.open(path)
            img.load()
        except Exception as err:            # ImageError / io::Error
            raise ReconstructionError(f"Failed to load source image: {err}") from err
        if focal_length_35mm is None:
            focal_length_35mm = SourceImage.get_focal_length_35mm(img)
        img = ImageOps.exif_transpose(img)  # decoder.orientation() + apply_orientation (:103-105)
        original_size = img.size
        img = img.convert("RGB")
        if img.size != (size, size) and resampler == "device":   # resize_exact(.., Lanczos3) (:107-113)
            if ctx is None:
                raise ReconstructionError("Failed to load source image: the device resampler needs a context")
            ctx = ctx() if callable(ctx) else ctx
            return SourceImage(ctx.resize_lanczos3(np.asarray(img, dtype=np.uint8), (size, size)), original_size,
                               focal_length_35mm)
        if img.size != (size, size):
            img = img.resize((size, size), Image.LANCZOS)
        return SourceImage(np.ascontiguousarray(np.asarray(img, dtype=np.uint8)), original_size,
                           focal_length_35mm)

    @staticmethod
    def _load_on_device(kind, path, focal_length_35mm, size, resampler, ctx, jpeg_entropy="host") -> "SourceImage":
        """kind "jpeg" or "png": the file decoded, oriented and (device resampler) resized on `ctx`"""
        import io
        from PIL import Image
        if ctx is None:
            raise ReconstructionError(f"Failed to load source image: the device {kind.upper()} decoder needs a context")
        try:
            with open(path, "rb") as f:
                data = f.read()
            ctx = ctx() if callable(ctx) else ctx
            if kind == "jpeg":
                ctx.set_jpeg_entropy(jpeg_entropy)
            width, height, _, _ = ctx._photo_info(f"me_{kind}_info", data)
            orientation = 1
            try:                                  # header only: Pillow parses the EXIF block, not the scans
                head = Image.open(io.BytesIO(data))
                if focal_length_35mm is None:
                    focal_length_35mm = SourceImage.get_focal_length_35mm(head)
                orientation = int(head.getexif().get(0x0112, 1))
            except Exception:
                pass
            if not 1 <= orientation <= 8:
                orientation = 1
            original_size = (height, width) if orientation >= 5 else (width, height)
            if resampler == "device":
                rgb = ctx._decode_photo_resized(kind, data, (size, size), orientation)   # :95-113 in one call
            else:
                img = Image.fromarray(ctx._decode_photo(kind, data, orientation))
                if img.size != (size, size):
                    img = img.resize((size, size), Image.LANCZOS)
                rgb = np.ascontiguousarray(np.asarray(img, dtype=np.uint8))
        except ReconstructionError:
            raise
        except Exception as err:
            raise ReconstructionError(f"Failed to load source image: {err}") from err
        return SourceImage(rgb, original_size, focal_length_35mm)

    @staticmethod
    def get_focal_length_35mm(img) -> Optional[float]:
        """reconstruction.rs:133-143"""
        try:
            exif = img.getexif()
            value = exif.get_ifd(_EXIF_IFD).get(_FOCAL_LENGTH_35MM, exif.get(_FOCAL_LENGTH_35MM))
        except Exception:
            return None
        return float(value) if value is not None else None     # the reference keeps Some(0) (reconstruction.rs:136-143)

    def focal_length_px(self) -> Optional[float]:
        """reconstruction.rs:145-152: f_img / f_35mm == diagonal / diagonal(24 mm x 36 mm)"""
        if self.focal_length_35mm is None:
            return None
        diagonal_35mm = math.sqrt(24.0 * 24.0 + 36.0 * 36.0)
        w, h = float(self.original_size[0]), float(self.original_size[1])
        return float(self.focal_length_35mm) * math.sqrt(w * w + h * h) / diagonal_35mm


def extract_depth(device: int, model_loader: DepthProModelLoader, source_path: str, destination_path: str,
                  focal_length_35mm: Optional[float], image_format: ImageOutputFormat,
                  vertex_mode: VertexMode, progress=None, noise=None, resampler=None, jpeg_decoder=None,
                  jpeg_entropy=None, png_decoder=None) -> None:
    """reconstruction.rs:155-205.  resampler: depth_pro.resolve_resampler, passed down to every resize; jpeg_decoder:
    depth_pro.resolve_jpeg_decoder, for the source photo, and jpeg_entropy: depth_pro.resolve_jpeg_entropy, for its
    Huffman decoding; png_decoder: depth_pro.resolve_png_decoder, for a .png source photo"""
    resampler = resolve_resampler(resampler)
    png_decoder = resolve_png_decoder(png_decoder)
    jpeg_decoder = resolve_jpeg_decoder(jpeg_decoder)
    jpeg_entropy = resolve_jpeg_entropy(jpeg_entropy)
    dtype = os.environ.get("MATRIX_EYES_DTYPE", "f16")   # f16 | bf16 | fp8, as the C++ twin
    try:
        img = SourceImage.load(source_path, focal_length_35mm, model_loader.cfg.img_size, resampler=resampler,
                               ctx=lambda: model_loader.context(device, dtype), jpeg_decoder=jpeg_decoder,
                               jpeg_entropy=jpeg_entropy, png_decoder=png_decoder)
    except ReconstructionError as err:
        print(err, file=sys.stderr)
        raise
    f_px = img.focal_length_px()
    f_norm = None if f_px is None else float(np.float32(f_px / float(img.original_size[0])))   # :174-176
    ctx = model_loader.context(device, dtype)
    ctx.set_progress(progress)
    try:
        inverse_depth = ctx.extract_depth(img.rgb8[None], f_norm)[0]
    except Exception as err:
        print(f"Failed to process image: {err}", file=sys.stderr)
        raise
    finally:
        ctx.set_progress(None)
    depth_map = DepthMap(ctx, inverse_depth, img.original_size)
    try:
        depth_map.output_image(destination_path, source_path, image_format, vertex_mode, noise=noise,
                               resampler=resampler)
    except Exception as err:
        print(f"Failed to output result: {err}", file=sys.stderr)
        raise
