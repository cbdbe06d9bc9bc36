"""Host-side mirror of the reference's `depth_pro` module interface over the C ABI.

reference src/depth_pro/mod.rs:
  pub const IMG_SIZE                                   (mod.rs:33)
  DepthProModelLoader::new(checkpoint_path, convert_checkpoints)   (mod.rs:167-172)
  DepthProModelLoader::extract_depth(img, f_norm, device, pl)      (mod.rs:251-363)
and the pub(super) module forwards the C ABI also exposes (vit.rs:328, encoder.rs:218,
decoder.rs:153, fov.rs:40).  Arrays are numpy (host) or torch CUDA tensors (device, zero copy).
"""
import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib as L
from .config import ModelConfig, expected_weights

IMG_SIZE = 384 * 4  # mod.rs:33


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _in_ptr(x, dtype):
    """(void* , keepalive) of a contiguous array of `dtype`; numpy -> host, torch -> its device."""
    if _is_torch(x):
        import torch
        want = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}[dtype]
        t = x if (x.dtype == want and x.is_contiguous()) else x.to(want).contiguous()
        return C.c_void_p(t.data_ptr()), t
    a = np.ascontiguousarray(x, dtype=dtype)
    return C.c_void_p(a.ctypes.data), a


def _out(out, shape, dtype=np.float32):
    """Output buffer: caller's torch/numpy array or a fresh numpy array."""
    if out is None:
        out = np.empty(shape, dtype=dtype)
    if _is_torch(out):
        assert out.is_contiguous() and tuple(out.shape) == tuple(shape), (out.shape, shape)
        return C.c_void_p(out.data_ptr()), out
    assert out.flags["C_CONTIGUOUS"] and out.shape == tuple(shape) and out.dtype == dtype
    return C.c_void_p(out.ctypes.data), out


def _resolve_choice(value, env_name, default, choices, what, alias=None):
    """`value`, or with None the environment's `env_name` (unset: `default`), if it is one of `choices`: itself, or what
    `alias` names for it.  Anything else is an argument error that calls the setting `what`."""
    if value is None:
        value = os.environ.get(env_name, default)
    if value not in choices:
        raise L.MatrixEyesError(1, f"{what} {value!r}: expected one of {', '.join(choices)}")
    return (alias or {}).get(value, value)


RESAMPLERS = ("pillow", "device")


def resolve_resampler(resampler=None) -> str:
    """Who makes the Lanczos3 resizes of reconstruction.rs:107-113 and output.rs:133-137, 206-218: "pillow" (the
    default: Pillow's filter, within one code of the reference's) or "device" (me_resize_lanczos3_rgb8: the `image`
    crate's sampler byte for byte, as the compiled CLI runs it).  None reads MATRIX_EYES_RESAMPLER; anything but the
    two names is an argument error."""
    return _resolve_choice(resampler, "MATRIX_EYES_RESAMPLER", "pillow", RESAMPLERS, "resampler")


PNG_ENCODERS = ("pillow", "device")


def resolve_png_encoder(png_encoder=None) -> str:
    """Who writes a ".png" destination (RgbImage::save, output.rs:138 and :192): "pillow" (the default) or "device"
    (me_output_png and the two whole-method calls: row filters, deflate and CRCs on the GPU, only the file's bytes come
    back).  The files decode to the same pixels.  None reads MATRIX_EYES_PNG_ENCODER; anything but the two names is an
    argument error."""
    return _resolve_choice(png_encoder, "MATRIX_EYES_PNG_ENCODER", "pillow", PNG_ENCODERS, "png encoder")


JPEG_ENCODERS = ("pillow", "host", "device")
JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def resolve_jpeg_encoder(jpeg_encoder=None) -> str:
    """Who writes a ".jpg" / ".jpeg" destination (RgbImage::save, output.rs:138 and :192): "pillow" (the default; "host",
    the compiled CLI's name for its own encoder, means the same here) or "device" (me_output_jpeg and the two whole-method
    calls: colour conversion, DCT, Huffman coding and byte stuffing on the GPU, only the file's bytes come back).  With the
    same quality and subsampling both write the same file, byte for byte.  None reads MATRIX_EYES_JPEG_ENCODER; anything
    but these names is an argument error."""
    return _resolve_choice(jpeg_encoder, "MATRIX_EYES_JPEG_ENCODER", "pillow", JPEG_ENCODERS, "jpeg encoder", {"host": "pillow"})


def resolve_jpeg_quality(jpeg_quality=None) -> int:
    """The quality a ".jpg" destination is written with, 1..100: None reads MATRIX_EYES_JPEG_QUALITY (default 75, Pillow's
    own); anything else is an argument error."""
    value = os.environ.get("MATRIX_EYES_JPEG_QUALITY", "75") if jpeg_quality is None else jpeg_quality
    try:
        quality = int(str(value).strip())
    except ValueError:
        quality = 0
    if not 1 <= quality <= 100:
        raise L.MatrixEyesError(1, f"jpeg quality {value!r}: expected an integer in 1..100")
    return quality


def resolve_jpeg_subsampling(jpeg_subsampling=None) -> int:
    """The chroma subsampling a ".jpg" destination is written with, as Pillow numbers it: "4:4:4" -> 0, "4:2:2" -> 1,
    "4:2:0" -> 2 (the numbers are accepted too).  None reads MATRIX_EYES_JPEG_SUBSAMPLING (default "4:2:0", Pillow's own);
    anything else is an argument error."""
    if not isinstance(jpeg_subsampling, (bool, str)) and jpeg_subsampling in (0, 1, 2):
        return int(jpeg_subsampling)
    return _resolve_choice(jpeg_subsampling, "MATRIX_EYES_JPEG_SUBSAMPLING", "4:2:0", JPEG_SUBSAMPLINGS, "jpeg subsampling",
                           JPEG_SUBSAMPLINGS)


JPEG_DECODERS = ("pillow", "host", "device")


def resolve_jpeg_decoder(jpeg_decoder=None) -> str:
    """Who decodes a ".jpg" / ".jpeg" source (reconstruction.rs:95-106): "pillow" (the default; "host", the compiled
    CLI's name for its own decoder, means the same here) or "device" (me_jpeg_decode_rgb8 / me_jpeg_decode_resized_rgb8:
    entropy decoding on the host, reconstruction and orientation on the GPU, the C++ host decoder's bytes).  None reads
    MATRIX_EYES_JPEG_DECODER; anything but these names is an argument error."""
    return _resolve_choice(jpeg_decoder, "MATRIX_EYES_JPEG_DECODER", "pillow", JPEG_DECODERS, "jpeg decoder", {"host": "pillow"})


PNG_DECODERS = ("pillow", "host", "device")


def resolve_png_decoder(png_decoder=None) -> str:
    """Who decodes a ".png" source (reconstruction.rs:95-106 for the photo, output.rs:206-218 for the vertex colours):
    "pillow" (the default; "host", the compiled CLI's name for its own decoder, means the same here) or "device"
    (me_png_decode_rgb8 / me_png_decode_resized_rgb8: zlib's inflate on the host, the scanline filters, the conversion to
    RGB, the de-interlacing and the orientation on the GPU, the compiled CLI's bytes).  None reads
    MATRIX_EYES_PNG_DECODER; anything but these names is an argument error."""
    return _resolve_choice(png_decoder, "MATRIX_EYES_PNG_DECODER", "pillow", PNG_DECODERS, "png decoder", {"host": "pillow"})


JPEG_ENTROPIES = ("host", "device")


def resolve_jpeg_entropy(jpeg_entropy=None) -> str:
    """Where the device JPEG decoder decodes the entropy-coded data: "host" (the default: the host decoder's loop on one
    core, the coefficients uploaded) or "device" (me_ctx_set_jpeg_entropy(ctx, 1): the scan's bytes uploaded and
    Huffman-decoded on the GPU; a file that decoder declines -- progressive, several scans, damaged -- takes the host loop).
    The same bytes either way.  Acts only with jpeg_decoder "device".  None reads MATRIX_EYES_JPEG_ENTROPY; anything but
    the two names is an argument error."""
    return _resolve_choice(jpeg_entropy, "MATRIX_EYES_JPEG_ENTROPY", "host", JPEG_ENTROPIES, "jpeg entropy decoder")


WEIGHT_PACKERS = ("host", "device")
WEIGHT_SOURCES = ("pt-host", "pt-device", "cache")


def resolve_weight_packer(weight_packer=None) -> str:
    """Who packs a checkpoint's tensors into the weight arena: "host" (the default: one core, one synchronous upload per
    tensor) or "device" (me_ctx_set_weight_packer(ctx, 1): raw bytes through a pinned ring, one pack kernel per tensor).
    The same arena bytes either way.  None reads MATRIX_EYES_WEIGHT_PACKER; anything but the two names is an argument
    error."""
    return _resolve_choice(weight_packer, "MATRIX_EYES_WEIGHT_PACKER", "host", WEIGHT_PACKERS, "weight packer")


NOISE_SOURCES = ("legacy", "host", "device")


def resolve_noise_source(noise_source=None) -> str:
    """Where a stereogram's noise comes from when the caller passes none: "legacy" (the default: numpy's PCG64 seeded with
    MATRIX_EYES_SEED or the OS, today's bytes), "host" (the keyed ChaCha12 noise of DESIGN.md §4.41 made by
    me_stereogram_noise_host on one core, then today's calls) or "device" (the keyed entries: the noise is made by a fill
    kernel in device scratch, no noise buffer exists on the host).  "host" and "device" write the same pixels for the same key.
    None reads MATRIX_EYES_NOISE; anything but the three names is an argument error."""
    return _resolve_choice(noise_source, "MATRIX_EYES_NOISE", "legacy", NOISE_SOURCES, "noise source")


def noise_key(lib, key=None) -> bytes:
    """The 32-byte key of the keyed noise: `key` itself, or -- None -- MATRIX_EYES_SEED as a full unsigned 64-bit decimal
    expanded by me_noise_key_from_seed; unset: 32 bytes from the OS (os.urandom)."""
    if key is not None:
        key = bytes(key)
        if len(key) != 32:
            raise L.MatrixEyesError(1, f"noise key: 32 bytes expected, got {len(key)}")
        return key
    seed = os.environ.get("MATRIX_EYES_SEED")
    if not seed:
        return os.urandom(32)
    if not (seed.isascii() and seed.isdigit()) or int(seed) >= 1 << 64:
        raise L.MatrixEyesError(1, f"MATRIX_EYES_SEED={seed}: expected an unsigned 64-bit decimal number")
    buf = (C.c_uint8 * 32)()
    rc = lib.me_noise_key_from_seed(int(seed), buf)
    if rc != L.ME_OK:
        raise L.MatrixEyesError(rc, "me_noise_key_from_seed")
    return bytes(buf)


class _DevMem:
    """`nbytes` of device memory at `ptr`, as torch.as_tensor takes it"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def _device_file(ptr, n, rgb):
    """The context-owned file of `n` bytes at `ptr` for the caller who passed `rgb`: numpy in -> `bytes`; a CUDA torch
    tensor in -> a CUDA uint8 tensor on its device (a copy)."""
    import torch
    on_device = _is_torch(rgb) and rgb.is_cuda
    file = torch.as_tensor(_DevMem(int(ptr.value), int(n.value)), device=rgb.device if on_device else "cuda")
    return file.clone() if on_device else file.cpu().numpy().tobytes()


class Context:
    """One GPU: stream, packed weights, workspaces (`me_ctx`)."""

    def __init__(self, device_id: int = 0, dtype: str = "f16", cfg: Optional[ModelConfig] = None, weight_packer: str = "host"):
        if weight_packer not in WEIGHT_PACKERS:
            raise L.MatrixEyesError(1, f"weight packer {weight_packer!r}: expected one of {', '.join(WEIGHT_PACKERS)}")
        self.lib = L.load_library()
        self.cfg = cfg or ModelConfig()
        self.dtype = dtype
        self._h = C.c_void_p()
        ccfg = self.cfg.to_c()
        code = {"f16": L.ME_DTYPE_F16, "bf16": L.ME_DTYPE_BF16, "fp8": L.ME_DTYPE_FP8}[dtype]
        rc = self.lib.me_ctx_create(device_id, code, C.byref(ccfg), C.byref(self._h))
        if rc != L.ME_OK:
            raise L.MatrixEyesError(rc, self.lib.me_last_error(None).decode())
        self._progress_ref = None
        if weight_packer == "device":
            self.set_weight_packer("device")

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.me_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        L.check(self.lib, self._h, rc)

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        self._check(self.lib.me_ctx_synchronize(self._h))

    def status_flags(self) -> int:
        """Status bits the kernels raised since the last call, read and cleared (matrix_eyes_hip.h ME_STATUS_*:
        1 = an f16 operand store met a magnitude beyond 65504)."""
        flags = C.c_uint32(0)
        self._check(self.lib.me_status_flags(self._h, C.byref(flags)))
        return int(flags.value)

    def calibrate(self):
        """The two fixed calibration loops (csrc/calibrate.hip): what THIS device gives on an MFMA-only loop and on a
        device copy -- bench.py prints it beside the step time so that runs on different boxes can be compared."""
        out = (C.c_double * 6)()
        self._check(self.lib.me_calibrate(self._h, out))
        return {"mfma_tflops": out[0], "mfma_clock_ghz": out[1], "copy_gbs": out[2], "mfma_loop_ms": out[3],
                "copy_ms": out[4], "cus": int(out[5])}

    def ln_fusion_state(self):
        """(fused, fallbacks): whether the ViT's residual launches still carry the LayerNorm behind them, and how many
        steps were run again on stand-alone LayerNorm launches after an ME_STATUS_SYNC_TIMEOUT
        (matrix_eyes_hip.h me_ln_fusion_state)."""
        fused, fallbacks = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.me_ln_fusion_state(self._h, C.byref(fused), C.byref(fallbacks)))
        return bool(fused.value), int(fallbacks.value)

    def last_mesh_timing(self):
        """legs of the last output_mesh(".obj", ".ply" or ".glb") call in ms: {mesh, format, d2h, file} and the file's size"""
        ms = (C.c_double * 4)()
        n = C.c_int64()
        self._check(self.lib.me_last_mesh_timing(self._h, ms, C.byref(n)))
        return {"mesh_ms": ms[0], "format_ms": ms[1], "d2h_ms": ms[2], "file_ms": ms[3], "bytes": int(n.value)}

    def set_output_overlap(self, on=True):
        """The output back end on a second stream, ordered behind the extract_depth call that wrote the depth buffer it
        reads (matrix_eyes_hip.h me_ctx_set_output_overlap): queue image i + 1's extract_depth, then make image i's
        DeviceDepthMap calls."""
        self._check(self.lib.me_ctx_set_output_overlap(self._h, 1 if on else 0))

    def set_write_behind(self, files_in_flight=2):
        """OBJ, PLY and GLB files written by host threads behind the caller, up to `files_in_flight` at a time; 0 / False: the
        synchronous form (matrix_eyes_hip.h me_ctx_set_write_behind)."""
        self._check(self.lib.me_ctx_set_write_behind(self._h, int(files_in_flight)))

    def output_flush(self):
        """Waits for every pending write-behind file; raises for a failed write (me_output_flush)."""
        self._check(self.lib.me_output_flush(self._h))

    def weight_arena_layout(self) -> int:
        """Hash of the weight arena's layout; contexts that exchange arenas must agree on it."""
        return int(self.lib.me_weight_arena_layout(self._h))

    def set_graph(self, on: bool = True):
        """Run device-pointer extract_depth calls as one captured hipGraph (matrix_eyes_hip.h me_ctx_set_graph)."""
        self._check(self.lib.me_ctx_set_graph(self._h, 1 if on else 0))

    @property
    def graph_launch_count(self) -> int:
        """extract_depth calls replayed from the captured hipGraph so far (matrix_eyes_hip.h)."""
        return int(self.lib.me_graph_launch_count(self._h))

    @property
    def side_branch_count(self) -> int:
        """extract_depth steps enqueued with the side branch forked (matrix_eyes_hip_ops.h me_side_branch_count)."""
        return int(self.lib.me_side_branch_count(self._h))

    def set_stream(self, hip_stream: Optional[int]):
        """Run on a caller-owned stream (its handle, e.g. torch.cuda.Stream().cuda_stream); None: the context's own.
        Handle 0, the legacy default stream, cannot be named (matrix_eyes_hip.h me_ctx_set_stream)."""
        self._check(self.lib.me_ctx_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def set_progress(self, fn):
        """fn(pos: float, message: Optional[str]) — ProgressListener (mod.rs:366-372)."""
        if fn is None:
            self._progress_ref = None
            self._check(self.lib.me_ctx_set_progress(self._h, L.PROGRESS_FN(0), None))
            return
        cb = L.PROGRESS_FN(lambda user, pos, msg: fn(pos, msg.decode() if msg else None))
        self._progress_ref = cb
        self._check(self.lib.me_ctx_set_progress(self._h, cb, None))

    def profile_enable(self, on: bool = True):
        self._check(self.lib.me_profile_enable(self._h, 1 if on else 0))

    def profile_report(self):
        import json
        buf = C.create_string_buffer(1 << 16)
        self._check(self.lib.me_profile_report(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    # -- weights (mod.rs:174-249 load_record)
    def expected_weights(self):
        n = self.lib.me_expected_weight_count(self._h)
        out = []
        name, dims, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int32()
        for i in range(n):
            self._check(self.lib.me_expected_weight(self._h, i, C.byref(name), dims, C.byref(nd)))
            out.append((name.value.decode(), tuple(dims[j] for j in range(nd.value))))
        return out

    def load_weight(self, name: str, tensor):
        """tensor: torch (f16/f32, CPU or CUDA) or numpy (float16/float32), PyTorch layout."""
        if _is_torch(tensor):
            import torch
            t = tensor.detach().contiguous()
            if t.dtype == torch.float16:
                wd = L.ME_WEIGHT_F16
            else:   # bf16, f64, integer buffers: through f32
                t, wd = t.to(torch.float32), L.ME_WEIGHT_F32
            ptr, shape, keep = C.c_void_p(t.data_ptr()), tuple(t.shape), t
        else:
            a = np.ascontiguousarray(tensor)
            if a.dtype == np.float16:
                wd = L.ME_WEIGHT_F16
            else:
                a, wd = a.astype(np.float32), L.ME_WEIGHT_F32
            ptr, shape, keep = C.c_void_p(a.ctypes.data), a.shape, a
        dims = (C.c_int64 * len(shape))(*shape)
        if _is_torch(tensor) and keep.is_cuda:
            # whatever torch still has queued that writes the tensor: the context's stream is not ordered behind torch's
            torch.cuda.current_stream(keep.device).synchronize()
        self._check(self.lib.me_load_weight(self._h, name.encode(), ptr, wd, dims, len(shape)))
        if _is_torch(tensor) and keep.is_cuda and keep.data_ptr() != tensor.data_ptr():
            # the device packer packs a device source where it lies, behind this call: a temporary copy made above must
            # outlive that launch (the caller's own tensor is the caller's to keep until finalize)
            self.synchronize()
        del keep

    def load_state_dict(self, state: Dict[str, object]):
        """Every tensor of `state` the model has a slot for, then me_weights_finalize (missing keys are errors:
        mod.rs:241-243).  Keys the model does not use are skipped and kept in `unused_keys`, as in the
        reference: each of its four parts is applied from the full snapshot list and only `result.errors` and
        `result.missing` are checked (mod.rs:236-243).  A tensor of the wrong shape stays an error."""
        expected = {n for n, _ in self.expected_weights()}
        self.unused_keys = [n for n in state if n not in expected]
        for name, t in state.items():
            if name in expected:
                self.load_weight(name, t)
        self._check(self.lib.me_weights_finalize(self._h))

    def load_checkpoint_pt(self, path: str):
        """me_load_checkpoint_pt: the library's own reader of `torch.save` archives (mod.rs:229-249)."""
        self._check(self.lib.me_load_checkpoint_pt(self._h, os.fsencode(path)))
        n = self.lib.me_unused_weight_count(self._h)
        self.unused_keys = [self.lib.me_unused_weight_name(self._h, i).decode() for i in range(n)]

    def set_weight_packer(self, who: str) -> None:
        """resolve_weight_packer's "host" / "device" for this context's weight loads (me_ctx_set_weight_packer)"""
        self._check(self.lib.me_ctx_set_weight_packer(self._h, 1 if resolve_weight_packer(who) == "device" else 0))

    def weight_cache_path(self, checkpoint_path: str) -> str:
        """The arena cache file's name for a checkpoint (me_weight_cache_path)"""
        buf = C.create_string_buffer(len(os.fsencode(checkpoint_path)) + 64)
        n = self.lib.me_weight_cache_path(self._h, os.fsencode(checkpoint_path), buf, len(buf))
        if n < 0:
            raise L.MatrixEyesError(1, "me_weight_cache_path failed")
        return os.fsdecode(buf.value)

    def save_weight_arena(self, path: str, source_path: Optional[str] = None) -> None:
        self._check(self.lib.me_save_weight_arena(self._h, os.fsencode(path), os.fsencode(source_path) if source_path else None))

    def load_weight_arena(self, path: str, source_path: Optional[str] = None) -> None:
        self._check(self.lib.me_load_weight_arena(self._h, os.fsencode(path), os.fsencode(source_path) if source_path else None))

    def load_checkpoint_cached(self, checkpoint_path: str, convert: bool = False) -> str:
        """me_load_checkpoint_cached, the policy of --convert-checkpoints; returns where the weights came from: one of
        WEIGHT_SOURCES"""
        where = C.c_int32(-1)
        self._check(self.lib.me_load_checkpoint_cached(self._h, os.fsencode(checkpoint_path), 1 if convert else 0, C.byref(where)))
        self.unused_keys = []                      # the cache holds the arena only: the checkpoint's keys were not read
        if where.value != 2:
            n = self.lib.me_unused_weight_count(self._h)
            self.unused_keys = [self.lib.me_unused_weight_name(self._h, i).decode() for i in range(n)]
        return WEIGHT_SOURCES[where.value]

    def last_weight_load(self):
        """(report, ms) of me_last_weight_load: report a dict of where (one of WEIGHT_SOURCES), tensors, bytes_read,
        bytes_uploaded; ms a dict of the five legs stage, upload, pack, finalize, cache_write"""
        info, ms = (C.c_int64 * 4)(), (C.c_double * 5)()
        self._check(self.lib.me_last_weight_load(self._h, info, ms))
        return ({"where": WEIGHT_SOURCES[info[0]], "tensors": int(info[1]), "bytes_read": int(info[2]), "bytes_uploaded": int(info[3])},
                dict(zip(("stage", "upload", "pack", "finalize", "cache_write"), (float(v) for v in ms))))

    def weight_arena_bytes(self) -> int:
        return int(self.lib.me_weight_arena_bytes(self._h))

    def weight_arena_tensor(self):
        """The packed weight arena as a zero-copy uint8 torch tensor on this context's GPU (for a
        caller-side collective)."""
        import torch
        ptr = self.lib.me_weight_arena_ptr(self._h)
        return torch.as_tensor(_DevMem(int(ptr), self.weight_arena_bytes()), device="cuda")

    def adopt_weights(self):
        self._check(self.lib.me_weights_adopt(self._h))

    def bcast_weights(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(unique_id, 128)
        self._check(self.lib.me_bcast_weights(self._h, buf, rank, nranks))

    def rccl_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self.lib.me_rccl_unique_id(buf)
        if rc != L.ME_OK:
            raise L.MatrixEyesError(rc, "ncclGetUniqueId failed")
        return buf.raw

    # -- forwards
    def preprocess_u8(self, rgb, out=None):
        B = rgb.shape[0]
        S = self.cfg.img_size
        p, keep = _in_ptr(rgb, np.uint8)
        po, out = _out(out, (B, 3, S, S))
        self._check(self.lib.me_preprocess_u8(self._h, p, B, po))
        return out

    def resize_lanczos3(self, rgb, size, out=None):
        """DynamicImage::resize_exact(nw, nh, Lanczos3) (reconstruction.rs:107-113, output.rs:133-137, 206-218) on the
        GPU, the `image` crate's bytes.  rgb: uint8 [h, w, 3], numpy (-> numpy) or a CUDA torch tensor (-> a CUDA
        tensor, queued on the context's stream, no host copy); size = (nw, nh)."""
        nw, nh = int(size[0]), int(size[1])
        if len(rgb.shape) != 3 or rgb.shape[2] != 3:
            raise L.MatrixEyesError(2, f"resize_lanczos3: uint8 [h, w, 3] expected, got {tuple(rgb.shape)}")
        if nw <= 0 or nh <= 0:
            raise L.MatrixEyesError(2, f"resize_lanczos3: target size {nw}x{nh}")
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        p, keep = _in_ptr(rgb, np.uint8)
        if out is None and _is_torch(rgb) and rgb.is_cuda:
            import torch
            out = torch.empty((nh, nw, 3), dtype=torch.uint8, device=rgb.device)
        po, out = _out(out, (nh, nw, 3), np.uint8)
        self._check(self.lib.me_resize_lanczos3_rgb8(self._h, p, w, h, po, nw, nh))
        return out

    @staticmethod
    def _photo_info(symbol: str, data: bytes):
        """me_jpeg_info / me_png_info: (width, height, exif_offset, exif_nbytes) of a file in memory"""
        lib = L.load_library()
        data = bytes(data)
        w, h, off, n = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        rc = getattr(lib, symbol)(data, len(data), C.byref(w), C.byref(h), C.byref(off), C.byref(n))
        if rc != L.ME_OK:
            msg = lib.me_last_error(None)
            raise L.MatrixEyesError(rc, msg.decode("utf-8", "replace") if msg else "")
        return w.value, h.value, off.value, n.value

    def _decode_photo(self, kind: str, data: bytes, orientation: int = 1, out=None):
        """me_jpeg_decode_rgb8 / me_png_decode_rgb8 (kind "jpeg" / "png") into `out` or a new numpy array"""
        data = bytes(data)
        w, h, _, _ = self._photo_info(f"me_{kind}_info", data)
        if 5 <= int(orientation) <= 8:
            w, h = h, w
        po, out = _out(out, (h, w, 3), np.uint8)
        self._check(getattr(self.lib, f"me_{kind}_decode_rgb8")(self._h, data, len(data), int(orientation), po, w, h))
        return out

    def _decode_photo_resized(self, kind: str, data: bytes, size, orientation: int = 1, out=None):
        """me_jpeg_decode_resized_rgb8 / me_png_decode_resized_rgb8 (kind "jpeg" / "png") to size = (nw, nh)"""
        data = bytes(data)
        nw, nh = int(size[0]), int(size[1])
        if nw <= 0 or nh <= 0:
            raise L.MatrixEyesError(2, f"decode_{kind}_resized: target size {nw}x{nh}")
        po, out = _out(out, (nh, nw, 3), np.uint8)
        self._check(getattr(self.lib, f"me_{kind}_decode_resized_rgb8")(self._h, data, len(data), int(orientation), po, nw, nh))
        return out

    @staticmethod
    def jpeg_info(data: bytes):
        """(width, height, exif_offset, exif_nbytes) of a JPEG file in memory (me_jpeg_info): the size as coded, before
        any orientation, and the span of the TIFF-structured EXIF block inside `data` (0, 0: none).  No GPU."""
        return Context._photo_info("me_jpeg_info", data)

    def decode_jpeg(self, data: bytes, orientation: int = 1, out=None):
        """The picture of a JPEG file, oriented (me_jpeg_decode_rgb8): uint8 [h, w, 3], the C++ host decoder's bytes.
        out: a numpy array or a CUDA torch tensor of the oriented shape (a CUDA one is only queued on the context's
        stream); None: a new numpy array."""
        return self._decode_photo("jpeg", data, orientation, out)

    def decode_jpeg_resized(self, data: bytes, size, orientation: int = 1, out=None):
        """decode_jpeg into context-owned device memory, then resize_lanczos3 to size = (nw, nh)
        (me_jpeg_decode_resized_rgb8, reconstruction.rs:95-113 in one call): only the resized picture leaves the device,
        or, with a CUDA `out`, nothing does."""
        return self._decode_photo_resized("jpeg", data, size, orientation, out)

    def set_jpeg_entropy(self, where: str) -> None:
        """resolve_jpeg_entropy's "host" / "device" for this context's JPEG decodes (me_ctx_set_jpeg_entropy)"""
        self._check(self.lib.me_ctx_set_jpeg_entropy(self._h, 1 if resolve_jpeg_entropy(where) == "device" else 0))

    def last_jpeg_entropy(self):
        """(report, ms) of me_last_jpeg_entropy: report a dict of where ("host" / "device"), reason, segments, subseqs,
        subseq_bits, rounds, upload_bytes, workgroups; ms (marker scan, upload, entropy kernels)"""
        rep, ms = (C.c_int64 * 8)(), (C.c_double * 3)()
        self._check(self.lib.me_last_jpeg_entropy(self._h, rep, ms))
        names = ("where", "reason", "segments", "subseqs", "subseq_bits", "rounds", "upload_bytes", "workgroups")
        out = dict(zip(names, (int(v) for v in rep)))
        out["where"] = "device" if out["where"] == 1 else "host"
        return out, tuple(float(v) for v in ms)

    def last_jpeg_timing(self):
        """[entropy decode (host), upload, IDCT kernel, finish kernel, download] of the last decode, in ms"""
        ms = (C.c_double * 5)()
        self._check(self.lib.me_last_jpeg_timing(self._h, ms))
        return list(ms)

    @staticmethod
    def png_info(data: bytes):
        """(width, height, exif_offset, exif_nbytes) of a PNG file in memory (me_png_info): IHDR's size, before any
        orientation, and the span of the last eXIf chunk's body inside `data` (0, 0: none).  No GPU."""
        return Context._photo_info("me_png_info", data)

    def decode_png(self, data: bytes, orientation: int = 1, out=None):
        """The picture of a PNG file, oriented (me_png_decode_rgb8): uint8 [h, w, 3], the C++ host decoder's bytes.
        out: a numpy array or a CUDA torch tensor of the oriented shape (a CUDA one is only queued on the context's
        stream); None: a new numpy array."""
        return self._decode_photo("png", data, orientation, out)

    def decode_png_resized(self, data: bytes, size, orientation: int = 1, out=None):
        """decode_png into context-owned device memory, then resize_lanczos3 to size = (nw, nh)
        (me_png_decode_resized_rgb8, reconstruction.rs:95-113 in one call): only the resized picture leaves the device,
        or, with a CUDA `out`, nothing does."""
        return self._decode_photo_resized("png", data, size, orientation, out)

    def last_png_timing(self):
        """[inflate (host), uploads, unfilter launches, finish kernel, download] of the last PNG decode, in ms"""
        ms = (C.c_double * 5)()
        self._check(self.lib.me_last_png_timing(self._h, ms))
        return list(ms)

    def op_png_unfilter(self, stream, width, height, bit_depth, colour_type, interlace=0, band_rows=0, out=None):
        """me_op_png_unfilter: the filtered stream of a PNG picture (uint8 [n], numpy or a CUDA tensor) -> the
        reconstructed stream in the same layout; band_rows 0: the default"""
        p, keep = _in_ptr(stream, np.uint8)
        n = int(stream.shape[0])
        if out is None and _is_torch(stream) and stream.is_cuda:
            import torch
            out = torch.empty((n,), dtype=torch.uint8, device=stream.device)
        po, out = _out(out, (n,), np.uint8)
        self._check(self.lib.me_op_png_unfilter(self._h, p, n, int(width), int(height), int(bit_depth), int(colour_type),
                                                int(interlace), int(band_rows), po))
        return out

    @staticmethod
    def _rgb_shape(rgb, who):
        if len(rgb.shape) != 3 or rgb.shape[2] != 3:
            raise L.MatrixEyesError(2, f"{who}: uint8 [h, w, 3] expected, got {tuple(rgb.shape)}")
        return int(rgb.shape[0]), int(rgb.shape[1])

    def png_encode(self, rgb):
        """RgbImage::save to ".png" without the file (me_png_encode_rgb8): uint8 [h, w, 3] -> the complete PNG file,
        encoded on the GPU.  numpy in -> `bytes`; a CUDA torch tensor in -> a CUDA uint8 tensor (a copy of the
        context-owned buffer)."""
        h, w = self._rgb_shape(rgb, "png_encode")
        p, keep = _in_ptr(rgb, np.uint8)
        ptr, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.me_png_encode_rgb8(self._h, p, w, h, C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, rgb)

    def output_png(self, rgb, destination_path: str):
        """png_encode, copied to the host once and written to destination_path (me_output_png)"""
        h, w = self._rgb_shape(rgb, "output_png")
        p, keep = _in_ptr(rgb, np.uint8)
        self._check(self.lib.me_output_png(self._h, p, w, h, str(destination_path).encode()))

    def jpeg_encode(self, rgb, quality: int = 75, subsampling: int = 2):
        """RgbImage::save to ".jpg" without the file (me_jpeg_encode_rgb8): uint8 [h, w, 3] -> the complete baseline JPEG
        file, encoded on the GPU; subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0.  numpy in -> `bytes`; a CUDA torch tensor
        in -> a CUDA uint8 tensor (a copy of the context-owned buffer)."""
        h, w = self._rgb_shape(rgb, "jpeg_encode")
        p, keep = _in_ptr(rgb, np.uint8)
        ptr, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.me_jpeg_encode_rgb8(self._h, p, w, h, int(quality), int(subsampling), C.byref(ptr), C.byref(n)))
        return _device_file(ptr, n, rgb)

    def output_jpeg(self, rgb, destination_path: str, quality: int = 75, subsampling: int = 2):
        """jpeg_encode, copied to the host once and written to destination_path (me_output_jpeg)"""
        h, w = self._rgb_shape(rgb, "output_jpeg")
        p, keep = _in_ptr(rgb, np.uint8)
        self._check(self.lib.me_output_jpeg(self._h, p, w, h, int(quality), int(subsampling), str(destination_path).encode()))

    def last_jpeg_encode(self):
        """me_last_jpeg_encode: (dict of blocks, scan_bits, stuffed, file_bytes, fdct_groups, wave_groups,
        block_scan_groups, stuff_groups, stuff_scan_groups, capacity; ms (upload, fdct, bits + scan, pack, stuffing,
        download))"""
        rep, ms = (C.c_int64 * 10)(), (C.c_double * 6)()
        self._check(self.lib.me_last_jpeg_encode(self._h, rep, ms))
        names = ("blocks", "scan_bits", "stuffed", "file_bytes", "fdct_groups", "wave_groups", "block_scan_groups",
                 "stuff_groups", "stuff_scan_groups", "capacity")
        return dict(zip(names, (int(v) for v in rep))), tuple(float(v) for v in ms)

    def vit_forward_features(self, which: int, xs, intermediate_blocks: Sequence[int] = ()):
        """vit.rs:328-346 -> (final [W,T,C], [intermediate ...])"""
        W = xs.shape[0]
        T, Cd = self.cfg.tokens, self.cfg.embed_dim
        p, keep = _in_ptr(xs, np.float32)
        n = len(intermediate_blocks)
        blocks = (C.c_int32 * max(n, 1))(*intermediate_blocks)
        final = np.empty((W, T, Cd), np.float32)
        inter = [np.empty((W, T, Cd), np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in inter])
        self._check(self.lib.me_vit_forward_features(self._h, which, p, W, blocks, n,
                                                     C.c_void_p(final.ctypes.data), ptrs))
        return final, inter

    def _enc_shapes(self, B):
        c, S = self.cfg, self.cfg.img_size
        return [(B, c.dec_dim, S // 2, S // 2), (B, c.enc_dims[0], S // 4, S // 4),
                (B, c.enc_dims[1], S // 8, S // 8), (B, c.enc_dims[2], S // 16, S // 16),
                (B, c.enc_dims[3], S // 32, S // 32)]

    def encoder_forward_encodings(self, x):
        """encoder.rs:218-335 -> 5 NCHW f32 arrays"""
        B = x.shape[0]
        p, keep = _in_ptr(x, np.float32)
        outs = [np.empty(s, np.float32) for s in self._enc_shapes(B)]
        ptrs = (C.c_void_p * 5)(*[a.ctypes.data for a in outs])
        self._check(self.lib.me_encoder_forward_encodings(self._h, p, B, ptrs))
        return outs

    def decoder_forward(self, encodings):
        """decoder.rs:153-208 -> (features, lowres_features)"""
        if len(encodings) != 5:   # decoder.rs:161-165
            raise L.MatrixEyesError(2, f"got encoder output levels {len(encodings)}, expected levels 5")
        B = encodings[0].shape[0]
        keep = [_in_ptr(e, np.float32) for e in encodings]
        ptrs = (C.c_void_p * 5)(*[k[0].value for k in keep])
        shapes = self._enc_shapes(B)
        feat = np.empty(shapes[0], np.float32)
        low = np.empty((B, self.cfg.dec_dim) + shapes[4][2:], np.float32)
        self._check(self.lib.me_decoder_forward(self._h, ptrs, B, C.c_void_p(feat.ctypes.data),
                                                C.c_void_p(low.ctypes.data)))
        return feat, low

    def head_forward(self, features):
        """mod.rs:323-338 -> canonical inverse depth [B,S,S]"""
        B, S = features.shape[0], self.cfg.img_size
        p, keep = _in_ptr(features, np.float32)
        out = np.empty((B, S, S), np.float32)
        self._check(self.lib.me_head_forward(self._h, p, B, C.c_void_p(out.ctypes.data)))
        return out

    def fov_forward(self, x, lowres_feature):
        """fov.rs:40-88 -> fov_deg [B]"""
        B = x.shape[0]
        p, k1 = _in_ptr(x, np.float32)
        pl, k2 = _in_ptr(lowres_feature, np.float32)
        out = np.empty((B,), np.float32)
        self._check(self.lib.me_fov_forward(self._h, p, pl, B, C.c_void_p(out.ctypes.data)))
        return out

    def extract_depth(self, img, f_norm=None, out=None, want_fov=False):
        """mod.rs:251-363.  img: f32 [B,3,S,S] or u8 [B,S,S,3]; f_norm: None (FOV head), a float,
        or [B] floats.  Returns inverse depth [B,S,S] (and fov_deg [B] when want_fov)."""
        S = self.cfg.img_size
        is_u8 = (img.dtype == np.uint8) if not _is_torch(img) else (str(img.dtype) == "torch.uint8")
        B = img.shape[0]
        p, keep = _in_ptr(img, np.uint8 if is_u8 else np.float32)
        fn_ptr, fn_keep = C.c_void_p(0), None
        if f_norm is not None and _is_torch(f_norm) and f_norm.is_cuda:
            # [B] f32 on the device: nothing in the call touches the host (eligible for the captured graph)
            fn_keep = f_norm.float().contiguous().reshape(B)
            fn_ptr = C.c_void_p(fn_keep.data_ptr())
        elif f_norm is not None:
            fn_keep = np.ascontiguousarray(np.broadcast_to(np.asarray(f_norm, np.float32), (B,)))
            fn_ptr = C.c_void_p(fn_keep.ctypes.data)
        po, out = _out(out, (B, S, S))
        fov = np.empty((B,), np.float32) if (want_fov and f_norm is None) else None
        fov_ptr = C.c_void_p(fov.ctypes.data) if fov is not None else C.c_void_p(0)
        fn = self.lib.me_extract_depth_u8 if is_u8 else self.lib.me_extract_depth
        self._check(fn(self._h, p, B, fn_ptr, po, fov_ptr))
        return (out, fov) if want_fov else out


class DepthProModelLoader:
    """reference `depth_pro::DepthProModelLoader` (mod.rs:120-123,166-172).

    The reference re-opens the checkpoint and builds/drops each stage's modules per call
    (mod.rs:276-351); here the weights are loaded once into the context and stay resident.
    `checkpoint_path` may be a PyTorch `.pt` state dict (torch.load) — or None / "synthetic" for
    the seeded synthetic checkpoint used when depth_pro.pt is not available."""

    def __init__(self, checkpoint_path: Optional[str] = "./checkpoints/depth_pro.pt",
                 convert_checkpoints: bool = False, cfg: Optional[ModelConfig] = None):
        self.checkpoint_path = checkpoint_path
        # mod.rs:211-247: the converted file is the packed weight arena, "<stem>-<dtype>-<layout hash>.mearena" beside the
        # checkpoint (Context.load_checkpoint_cached); loaded whenever it is there and valid, written when this is set
        self.convert_checkpoints = convert_checkpoints
        self.cfg = cfg or ModelConfig()
        self._ctx = None

    def _state_dict(self):
        if self.checkpoint_path in (None, "synthetic"):
            from .synthetic import synthetic_checkpoint
            return synthetic_checkpoint(self.cfg)
        if not os.path.exists(self.checkpoint_path):
            # LoaderError::Pytorch (mod.rs:426)
            raise L.MatrixEyesError(7, f"Failed to load depth model: {self.checkpoint_path}: no such file")
        import torch
        state = torch.load(self.checkpoint_path, map_location="cpu", weights_only=True)
        return state.get("state_dict", state) if isinstance(state, dict) else state

    def context(self, device: int = 0, dtype: str = "f16") -> Context:
        if self._ctx is None:
            ctx = Context(device, dtype, self.cfg, weight_packer=resolve_weight_packer())
            if self.checkpoint_path in (None, "synthetic") or os.environ.get("ME_TORCH_LOAD"):
                ctx.load_state_dict(self._state_dict())
            else:
                # the arena cache beside the checkpoint if it is there and valid; otherwise the library maps and parses the
                # .pt archive itself (me_load_checkpoint_pt) and, with convert_checkpoints, writes the cache; ME_TORCH_LOAD=1
                # goes through torch.load instead
                ctx.load_checkpoint_cached(self.checkpoint_path, self.convert_checkpoints)
            self._ctx = ctx
        return self._ctx

    def extract_depth(self, img, f_norm: Optional[float], device: int = 0, pl=None, dtype="f16"):
        """img [1,3,1536,1536] f32 (reconstruction.rs:116-124 layout) -> inverse depth [1536,1536]
        (mod.rs:336-338 squeezes the batch: batch 1 only, like the reference)."""
        if img.shape[0] != 1:
            raise L.MatrixEyesError(2, "extract_depth: batch must be 1 (mod.rs:336-338)")
        ctx = self.context(device, dtype)
        ctx.set_progress(pl)
        try:
            return ctx.extract_depth(img, f_norm)[0]
        finally:
            ctx.set_progress(None)
