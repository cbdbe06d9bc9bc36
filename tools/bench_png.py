#!/usr/bin/env python3
"""Times the PNG encoder on the GPU against the host layer's encode_png work on one CPU core, one JSON line per picture:

  host_ms     what host/image_io.cpp encode_png does with the pixels in host memory: every row copied behind a filter
              byte 0, zlib's compress at level 6 (compress2(.., 6)), the IDAT CRC-32; same process, one core
  device_ms   me_png_encode_rgb8 from DEVICE-resident pixels plus the D2H copy of the finished file into pinned host
              memory: wall clock around both, a device synchronise inside the window
  host_bytes, device_bytes   the two files' sizes; raw_bytes = w * h * 3
  speedup     host_ms / device_ms

Pictures (tests/png_pictures.py, seeded): the library's own depth map (me_depthmap_rgb_resized) and stereogram
(me_stereogram) of a synthetic inverse-depth field, uniform noise, and a flat picture, at 1536 x 1536 and 4032 x 3024.
Every shape is warmed up, the two legs alternate, medians of --repeats (at least 10).  The kernel rows come from a
separate run under rocprofv3 --kernel-trace --stats (--device-only skips the host leg for that).

    python3 tools/bench_png.py [--repeats 10] [--sizes 1536x1536,4032x3024] [--out profiles/png_encode_ab.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_encode(rgb):
    """encode_png's work: filter 0, compress level 6, the CRC over type + data"""
    import numpy as np
    h = rgb.shape[0]
    rows = np.empty((h, 1 + rgb.shape[1] * 3), np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = rgb.reshape(h, -1)
    z = zlib.compress(rows.tobytes(), 6)
    zlib.crc32(z, zlib.crc32(b"IDAT"))
    return len(z) + 57


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sizes", default="1536x1536,4032x3024")
    ap.add_argument("--pictures", default="depth,stereogram,noise,flat")
    ap.add_argument("--device-only", action="store_true", help="no host leg (for a run under the profiler)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    import numpy as np
    import torch
    import matrix_eyes_amd as m
    import png_check
    import png_pictures as pic
    assert torch.cuda.is_available(), "bench_png needs a GPU"
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    lib, hd = ctx.lib, ctx.handle
    field = pic.inverse_depth_field(1536)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        dm = m.DepthMap(ctx, field, (w, h))
        for name in args.pictures.split(","):
            if name == "depth":
                rgb = dm.depth_map_rgb_resized()
            elif name == "stereogram":
                rgb = dm.stereogram(None, 1.0 / 16.0, pic.noise_picture(h, w, seed=21))
            elif name == "noise":
                rgb = pic.noise_picture(h, w, seed=33)
            else:
                rgb = pic.flat_picture(h, w)
            d_rgb = torch.from_numpy(rgb).cuda()
            pinned = torch.empty(rgb.size + rgb.size // 500 + 4096, dtype=torch.uint8).pin_memory()
            ptr, n = C.c_void_p(), C.c_int64()

            class DevMem:
                def __init__(self, address, nbytes):
                    self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (address, False), "version": 2}

            def device_leg():
                ctx._check(lib.me_png_encode_rgb8(hd, C.c_void_p(d_rgb.data_ptr()), w, h, C.byref(ptr), C.byref(n)))
                file = torch.as_tensor(DevMem(int(ptr.value), int(n.value)), device="cuda")
                pinned[:n.value].copy_(file, non_blocking=True)
                torch.cuda.synchronize()
                return n.value

            torch.cuda.synchronize()
            nbytes = device_leg()                                    # warm-up: scratch allocation
            device_leg()
            data = pinned[:nbytes].numpy().tobytes()
            px, _ = png_check.read_png(data)
            assert np.array_equal(px, rgb), "the device's file does not decode to the input"
            host_bytes = None if args.device_only else host_encode(rgb)
            dev_ms, host_ms = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                device_leg()                                         # ends in a device synchronise
                dev_ms.append((time.perf_counter() - t0) * 1e3)
                if not args.device_only:
                    t0 = time.perf_counter()
                    host_encode(rgb)
                    host_ms.append((time.perf_counter() - t0) * 1e3)
            row = dict(op="png_encode_rgb8", picture=name, size=f"{w}x{h}", raw_bytes=rgb.size, device_bytes=nbytes,
                       device_ms=round(statistics.median(dev_ms), 3), device_ms_min=round(min(dev_ms), 3),
                       device_ms_max=round(max(dev_ms), 3), repeats=args.repeats)
            if not args.device_only:
                hm = statistics.median(host_ms)
                row.update(host_bytes=host_bytes, host_ms=round(hm, 1), speedup=round(hm / row["device_ms"], 1),
                           device_over_host_bytes=round(nbytes / host_bytes, 3))
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
