#!/usr/bin/env python3
"""Times the PNG decoder on the GPU against the C++ host layer's decoder on one CPU core, one JSON line per form of file:

  host_ms            (a) host/png_decoder.cpp decode_png, through the library (me_op_png_decode_host): inflate, the scanline
                     filters byte by byte, the conversion to RGB, the copy into the caller's array; same process, one core
  host_inflate_ms    zlib's inflate of the file's IDAT data alone (Python's zlib.decompress: the same library), the share
                     of (a) that stays on the host in (b); host_recon_ms = host_ms - host_inflate_ms is what the GPU takes
  device_ms          (b) me_png_decode_rgb8 into a DEVICE buffer: wall clock around the call and a context synchronise
  device_host_ms     (b') the same into PINNED host memory: the call ends in a stream synchronise
  legs_ms            (b') split (me_last_png_timing): inflate on the host (wall clock, the uploads and launches are queued
                     from inside it), uploads, unfilter launches, finish kernel, download -- the four device legs by HIP
                     events, summed over the bands; legs_ms_range: each leg's smallest and largest value over the repeats
  hidden             whether the unfilter launches hide under the inflate: device_ms - legs_ms.inflate is what is left
                     behind the inflate's end (tail_ms)

Forms, all --size (4032 x 3024): 8-bit RGB with every row Paeth (the serial worst case); 8-bit RGB with the row filters
me_png_encode_rgb8 chooses for a photo-like picture; 16-bit RGB; interlaced 8-bit RGBA.  The hand-made files come from
tests/png_files.py.  Every leg is warmed up, the legs alternate, medians of --repeats (at least 10) with minimum and
maximum.  The device's picture is checked against the host's before anything is timed.

    python3 tools/bench_png_decode.py [--repeats 10] [--size 4032x3024] [--out profiles/png_decode_ab.txt]
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


def idat_of(data: bytes) -> bytes:
    z, pos = b"", 8
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        if data[pos + 4:pos + 8] == b"IDAT":
            z += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--size", default="4032x3024")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    import numpy as np
    import torch
    import matrix_eyes_amd as m
    import jpeg_files as J
    import png_files as P
    assert torch.cuda.is_available(), "bench_png_decode needs a GPU"
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    lib, hd = ctx.lib, ctx.handle
    w, h = (int(v) for v in args.size.split("x"))
    picture = J.photo(w, h, 41)
    p16 = picture.astype(np.uint16)
    rgba = np.concatenate([p16, np.full((h, w, 1), 255, np.uint16)], -1)
    forms = (("rgb8-all-paeth", lambda: P.make(w, h, 2, 8, 0, (4,), px=p16, level=1)),
             ("rgb8-encoder-filters", lambda: ctx.png_encode(picture)),
             ("rgb16", lambda: P.make(w, h, 2, 16, 0, (4, 1, 2, 3), px=p16 * 257, level=1)),
             ("rgba8-adam7", lambda: P.make(w, h, 6, 8, 1, (4, 1, 2, 3), px=rgba, level=1)))
    for form, make in forms:
        data = make()
        z = idat_of(data)
        host_out = np.empty((h, w, 3), np.uint8)
        pinned = torch.empty((h, w, 3), dtype=torch.uint8).pin_memory()
        dev = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")

        def host_leg():
            assert lib.me_op_png_decode_host(data, len(data), C.c_void_p(host_out.ctypes.data), w, h) == 0

        def device_leg():
            ctx._check(lib.me_png_decode_rgb8(hd, data, len(data), 1, C.c_void_p(dev.data_ptr()), w, h))
            ctx.synchronize()

        def device_host_leg():
            ctx._check(lib.me_png_decode_rgb8(hd, data, len(data), 1, C.c_void_p(pinned.data_ptr()), w, h))

        for _ in range(2):                                        # warm-up: scratch, pinned staging, events
            host_leg(), device_leg(), device_host_leg()
        for name, got in (("device", dev.cpu().numpy()), ("host", pinned.numpy())):
            bad = int((got != host_out).sum())
            assert bad == 0, f"{form}: {bad} bytes of the picture in {name} memory differ from the host decoder's"
        ha, hi, db, dh, legs = [], [], [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            host_leg()
            ha.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            zlib.decompress(z)
            hi.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            device_leg()
            db.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            device_host_leg()                                     # ends in a stream synchronise (a host destination)
            dh.append((time.perf_counter() - t0) * 1e3)
            legs.append(ctx.last_png_timing())
        med = statistics.median
        leg = [med([v[i] for v in legs]) for i in range(5)]
        tail = med(db) - leg[0]
        row = dict(op="png_decode_rgb8", form=form, size=f"{w}x{h}", file_bytes=len(data), repeats=args.repeats,
                   host_ms=round(med(ha), 1), host_ms_min=round(min(ha), 1), host_ms_max=round(max(ha), 1),
                   host_inflate_ms=round(med(hi), 1), host_recon_ms=round(med(ha) - med(hi), 1),
                   device_ms=round(med(db), 2), device_ms_min=round(min(db), 2), device_ms_max=round(max(db), 2),
                   device_host_ms=round(med(dh), 2), device_host_ms_min=round(min(dh), 2), device_host_ms_max=round(max(dh), 2),
                   legs_ms=dict(inflate=round(leg[0], 2), uploads=round(leg[1], 3), unfilter=round(leg[2], 3),
                                finish=round(leg[3], 3), download=round(leg[4], 3)),
                   legs_ms_range={k: [round(min(v[i] for v in legs), 3), round(max(v[i] for v in legs), 3)]
                                  for i, k in enumerate(("inflate", "uploads", "unfilter", "finish", "download"))},
                   tail_ms=round(tail, 2), hidden=bool(leg[2] > 2 * max(tail - leg[3], 0.0)),
                   device_recon_vs_host_recon=round((leg[2] + leg[3]) / max(med(ha) - med(hi), 1e-9), 3),
                   speedup=round(med(ha) / med(db), 2), speedup_to_host=round(med(ha) / med(dh), 2))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
