#!/usr/bin/env python3
"""Times the JPEG decoder on the GPU against the C++ host layer's decoder on one CPU core, one JSON line per file:

  host_ms            (a) host/jpeg_decoder.cpp decode_jpeg, through the library (me_op_jpeg_decode_host): entropy decoding,
                     IDCT, upsampling, colour conversion, the copy into the caller's array; same process, one core
  device_ms          (b) me_jpeg_decode_rgb8 into PINNED host memory: wall clock, the call ends in a stream synchronise
  legs_ms            (b) split (me_last_jpeg_timing): entropy decode on the host (wall clock), upload of the coefficients,
                     jpeg_idct_kernel, jpeg_finish_kernel, download -- the four device legs by HIP events
  legs_ms_range      (b) the smallest and largest value of each leg over the repeats
  resized_ms         (c) me_jpeg_decode_resized_rgb8 into a 1536 x 1536 DEVICE buffer: wall clock around the call and a
                     context synchronise
  entropy_share      legs_ms.entropy / device_ms: what is left on the host
  speedup_b, speedup_c   host_ms / device_ms, host_ms / resized_ms
  device_entropy_ms  (d) leg (b) with me_ctx_set_jpeg_entropy(ctx, 1): the scan's bytes uploaded and Huffman-decoded on the
                     GPU (csrc/jpeg_entropy.hip); a file that decoder declines (the progressive one) runs leg (b)'s path
  entropy_legs_ms    (d) split (me_last_jpeg_timing as above, and me_last_jpeg_entropy): marker scan and destuffing on the
                     host, upload of the scan, the entropy kernels; entropy_report: where, decline reason, segments,
                     subsequences, bits per subsequence, sync rounds, bytes uploaded, workgroups
  speedup_d, d_over_b    host_ms / device_entropy_ms, device_ms / device_entropy_ms

Files: 4032 x 3024, 4:2:0, quality 90, baseline and progressive, written by Pillow from the seeded photo of
tests/jpeg_files.py (= tests/test_gpu_resample.py photo()).  Every leg is warmed up, the four legs alternate, medians of
--repeats (at least 10).  The device's picture is checked against the host's before anything is timed.

    python3 tools/bench_jpeg.py [--repeats 10] [--size 4032x3024] [--out profiles/jpeg_decode_ab.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--size", default="4032x3024")
    ap.add_argument("--resized", type=int, default=1536)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    import numpy as np
    import torch
    import matrix_eyes_amd as m
    import jpeg_files as J
    assert torch.cuda.is_available(), "bench_jpeg needs a GPU"
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    lib, hd = ctx.lib, ctx.handle
    w, h = (int(v) for v in args.size.split("x"))
    picture = J.photo(w, h, 41)
    S = args.resized
    for scan in ("baseline", "progressive"):
        data = J.save(picture, quality=90, subsampling=2, progressive=scan == "progressive")
        host_out = np.empty((h, w, 3), np.uint8)
        pinned = torch.empty((h, w, 3), dtype=torch.uint8).pin_memory()
        resized = torch.empty((S, S, 3), dtype=torch.uint8, device="cuda")

        def host_leg():
            assert lib.me_op_jpeg_decode_host(data, len(data), C.c_void_p(host_out.ctypes.data), w, h) == 0

        def device_leg():
            ctx._check(lib.me_jpeg_decode_rgb8(hd, data, len(data), 1, C.c_void_p(pinned.data_ptr()), w, h))

        def resized_leg():
            ctx._check(lib.me_jpeg_decode_resized_rgb8(hd, data, len(data), 1, C.c_void_p(resized.data_ptr()), S, S))
            ctx.synchronize()

        def device_entropy_leg():
            ctx.set_jpeg_entropy("device")
            try:
                device_leg()
            finally:
                ctx.set_jpeg_entropy("host")

        for _ in range(2):                                        # warm-up: scratch, pinned staging, resampler tables
            host_leg(), device_leg(), resized_leg()
        bad = int((pinned.numpy() != host_out).sum())
        assert bad == 0, f"{bad} bytes of the device's picture differ from the host decoder's"
        for _ in range(2):
            pinned.zero_()
            device_entropy_leg()
        bad = int((pinned.numpy() != host_out).sum())
        assert bad == 0, f"{bad} bytes of the picture differ from the host decoder's with the entropy leg on the device"
        ha, db, rc, legs = [], [], [], []
        de, dlegs, elegs, report = [], [], [], None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            host_leg()
            ha.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            device_leg()                                          # ends in a stream synchronise (a host destination)
            db.append((time.perf_counter() - t0) * 1e3)
            legs.append(ctx.last_jpeg_timing())
            t0 = time.perf_counter()
            resized_leg()
            rc.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            device_entropy_leg()
            de.append((time.perf_counter() - t0) * 1e3)
            dlegs.append(ctx.last_jpeg_timing())
            report, ems = ctx.last_jpeg_entropy()
            elegs.append(ems)
        med = statistics.median
        leg = [med([v[i] for v in legs]) for i in range(5)]
        row = dict(op="jpeg_decode_rgb8", scan=scan, size=f"{w}x{h}", file_bytes=len(data), repeats=args.repeats,
                   host_ms=round(med(ha), 1), device_ms=round(med(db), 2), device_ms_min=round(min(db), 2),
                   device_ms_max=round(max(db), 2),
                   legs_ms=dict(entropy=round(leg[0], 2), upload=round(leg[1], 3), idct=round(leg[2], 3),
                                finish=round(leg[3], 3), download=round(leg[4], 3)),
                   legs_ms_range={k: [round(min(v[i] for v in legs), 3), round(max(v[i] for v in legs), 3)]
                                  for i, k in enumerate(("entropy", "upload", "idct", "finish", "download"))},
                   resized_ms=round(med(rc), 2), resized_to=f"{S}x{S}",
                   entropy_share=round(leg[0] / med(db), 3),
                   speedup_b=round(med(ha) / med(db), 2), speedup_c=round(med(ha) / med(rc), 2))
        dleg = [med([v[i] for v in dlegs]) for i in range(5)]
        eleg = [med([v[i] for v in elegs]) for i in range(3)]
        row.update(device_entropy_ms=round(med(de), 2), device_entropy_ms_min=round(min(de), 2),
                   device_entropy_ms_max=round(max(de), 2),
                   entropy_legs_ms=dict(entropy=round(dleg[0], 2), marker_scan=round(eleg[0], 3), scan_upload=round(eleg[1], 3),
                                        entropy_kernels=round(eleg[2], 3), idct=round(dleg[2], 3), finish=round(dleg[3], 3),
                                        download=round(dleg[4], 3)),
                   entropy_report=report, speedup_d=round(med(ha) / med(de), 2), d_over_b=round(med(db) / med(de), 2))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
