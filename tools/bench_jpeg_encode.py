#!/usr/bin/env python3
"""Times the JPEG encoder, four legs alternating in one process, medians of --repeats (at least 10), one JSON line per case:

  host_ms      (a) me_op_jpeg_encode_host: the host layer's sequential encode_jpeg on one CPU core, pixels in host memory
  pillow_ms    (b) Pillow's Image.save(buf, "JPEG", quality, subsampling, optimize=False) from a host array (libjpeg-turbo
               where Pillow links it: its SIMD path), the yardstick of the same run
  device_ms    (c) me_jpeg_encode_rgb8 from DEVICE-resident pixels to the file in device memory (two synchronisations inside)
  output_ms    (d) me_output_jpeg from DEVICE-resident pixels to a file on disk, and the medians of its legs from
               me_last_jpeg_encode (HIP events): upload, fdct, bits + scan, pack, stuffing, download
  bytes        the file's size (all four write the same file; asserted before timing), raw_bytes = w * h * 3

Pictures: the library's own 1536 x 1536 depth picture (me_depthmap_rgb_resized of tests/png_pictures.py's field) at
quality 75 4:2:0, and the seeded 4032 x 3024 test photo (tests/jpeg_files.py photo) at quality 75 4:2:0 and 90 4:4:4.

    python3 tools/bench_jpeg_encode.py [--repeats 10] [--out profiles/jpeg_encode_ab.txt]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = ("upload", "fdct", "bits_scan", "pack", "stuffing", "download")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cases", default="depth:75:2,photo:75:2,photo:90:0", help="picture:quality:subsampling, ...")
    ap.add_argument("--device-only", action="store_true", help="no host or Pillow leg (for a run under the profiler)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    import numpy as np
    import torch
    from PIL import Image, features
    import matrix_eyes_amd as m
    import jpeg_files
    import png_pictures as pic
    assert torch.cuda.is_available(), "bench_jpeg_encode needs a GPU"
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    lib, hd = ctx.lib, ctx.handle
    pictures = {}
    tmp = tempfile.mkdtemp(prefix="jpeg_encode_bench_")
    path = os.path.join(tmp, "out.jpg")
    for case in args.cases.split(","):
        name, quality, subsampling = case.split(":")
        quality, subsampling = int(quality), int(subsampling)
        if name not in pictures:
            if name == "depth":
                pictures[name] = m.DepthMap(ctx, pic.inverse_depth_field(1536), (1536, 1536)).depth_map_rgb_resized()
            else:
                pictures[name] = np.ascontiguousarray(jpeg_files.photo(4032, 3024, 9))
        rgb = pictures[name]
        h, w = rgb.shape[:2]
        d_rgb = torch.from_numpy(rgb).cuda()
        out = np.zeros(rgb.size + 4096, np.uint8)
        n, ptr = C.c_int64(), C.c_void_p()

        def host_leg():
            assert lib.me_op_jpeg_encode_host(C.c_void_p(rgb.ctypes.data), w, h, quality, subsampling, C.c_void_p(out.ctypes.data),
                                              out.size, C.byref(n)) == 0
            return out[:n.value].tobytes()

        def pillow_leg():
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=False)
            return buf.getvalue()

        def device_leg():
            ctx._check(lib.me_jpeg_encode_rgb8(hd, C.c_void_p(d_rgb.data_ptr()), w, h, quality, subsampling, C.byref(ptr), C.byref(n)))
            return n.value

        def output_leg():
            ctx._check(lib.me_output_jpeg(hd, C.c_void_p(d_rgb.data_ptr()), w, h, quality, subsampling, path.encode()))

        torch.cuda.synchronize()
        device_leg()                                                 # warm-up: scratch allocation
        output_leg()
        with open(path, "rb") as f:
            data = f.read()
        assert len(data) == device_leg()
        if not args.device_only:
            assert data == host_leg(), "the device's file differs from the host encoder's"
            if features.check_feature("libjpeg_turbo"):
                assert data == pillow_leg(), "the device's file differs from Pillow's"
        times = {k: [] for k in ("host", "pillow", "device", "output") + LEGS}
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            device_leg()
            times["device"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            output_leg()
            times["output"].append((time.perf_counter() - t0) * 1e3)
            for k, v in zip(LEGS, ctx.last_jpeg_encode()[1]):
                times[k].append(v)
            if not args.device_only:
                t0 = time.perf_counter()
                host_leg()
                times["host"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                pillow_leg()
                times["pillow"].append((time.perf_counter() - t0) * 1e3)
        rep = ctx.last_jpeg_encode()[0]
        med = {k: statistics.median(v) for k, v in times.items() if v}
        row = dict(op="jpeg_encode_rgb8", picture=name, size=f"{w}x{h}", quality=quality, subsampling=subsampling, raw_bytes=rgb.size,
                   bytes=len(data), blocks=rep["blocks"], stuffed=rep["stuffed"], device_ms=round(med["device"], 3),
                   device_ms_min=round(min(times["device"]), 3), device_ms_max=round(max(times["device"]), 3),
                   output_ms=round(med["output"], 3), legs_ms={k: round(med[k], 3) for k in LEGS}, repeats=args.repeats)
        if not args.device_only:
            row.update(host_ms=round(med["host"], 2), pillow_ms=round(med["pillow"], 2),
                       libjpeg_turbo=bool(features.check_feature("libjpeg_turbo")),
                       pillow_over_device=round(med["pillow"] / med["device"], 2), pillow_over_output=round(med["pillow"] / med["output"], 2))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    os.remove(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
