#!/usr/bin/env python3
"""Times the Lanczos3 resize (reconstruction.rs:107-113, output.rs:133-137) on one CPU core and on the GPU, one JSON
line per size pair:

  host_ms         the C++ host layer's loop (host/image_io.cpp resize_exact_lanczos3, what MATRIX_EYES_RESAMPLER=host
                  runs), timed inside `host_selftest resize-time` around the call alone: no files, no decode
  device_host_ms  me_resize_lanczos3_rgb8 with host pointers: wall clock around the call, which ends in a stream
                  synchronise; includes both copies through pageable memory (median of --host-iters)
  device_ms       the same entry with device pointers: hipEvents around one call, median of --iters after warm-up
  bytes_moved     what the two passes read and write once each: source + 2 x the f32 intermediate + result
  frac_of_hbm     bytes_moved / device_ms against 6.3 TB/s

    python3 tools/bench_resize.py [--pairs 4032x3024:1536x1536,...] [--iters 30] [--out profiles/resample_ab.txt]

Each pair's GPU part runs in a child process of its own under a time limit; the first failure ends the run.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SELFTEST = os.path.join(ROOT, "matrix-eyes_amd", "host_selftest")
DEFAULT_PAIRS = "4032x3024:1536x1536,1536x1536:4032x3024,6000x4000:1536x1536"
HBM_BYTES_PER_S = 6.3e12


def parse_pairs(text):
    pairs = []
    for item in text.split(","):
        a, b = item.split(":")
        pairs.append(tuple(int(v) for v in a.split("x")) + tuple(int(v) for v in b.split("x")))
    return pairs


def child(w, h, nw, nh, iters, host_iters):
    import numpy as np
    import torch
    import matrix_eyes_amd as m
    assert torch.cuda.is_available(), "bench_resize needs a GPU"
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    lib, hd = ctx.lib, ctx.handle
    img = np.random.default_rng(w * 31 + nh).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = np.empty((nh, nw, 3), np.uint8)
    src, dst = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)

    host_ms = []
    for k in range(host_iters + 1):                      # the first call allocates scratch and builds the tables
        t0 = time.perf_counter()
        ctx._check(lib.me_resize_lanczos3_rgb8(hd, src, w, h, dst, nw, nh))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    d_src = torch.from_numpy(img).cuda()
    d_dst = torch.empty((nh, nw, 3), dtype=torch.uint8, device="cuda")
    ps, pd = C.c_void_p(d_src.data_ptr()), C.c_void_p(d_dst.data_ptr())
    for _ in range(3):
        ctx._check(lib.me_resize_lanczos3_rgb8(hd, ps, w, h, pd, nw, nh))
    ctx.synchronize()
    dev_ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx._check(lib.me_resize_lanczos3_rgb8(hd, ps, w, h, pd, nw, nh))
        e1.record(stream)
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    assert np.array_equal(d_dst.cpu().numpy(), out), "device-pointer and host-pointer results differ"
    moved = w * h * 3 + 2 * w * nh * 3 * 4 + nw * nh * 3
    ms = statistics.median(dev_ms)
    print(json.dumps(dict(first_call_ms=round(host_ms[0], 3), device_host_ms=round(statistics.median(host_ms[1:]), 3),
                          device_ms=round(ms, 4), device_ms_min=round(min(dev_ms), 4), device_ms_max=round(max(dev_ms), 4),
                          iters=iters, bytes_moved=moved, frac_of_hbm=round(moved / (ms * 1e-3) / HBM_BYTES_PER_S, 4))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default=DEFAULT_PAIRS)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU loop (seconds per pair)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--child", nargs=4, type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.iters < 20:
            ap.error("--iters: at least 20")
        return child(*args.child, args.iters, args.host_iters)
    for w, h, nw, nh in parse_pairs(args.pairs):
        row = dict(op="resize_lanczos3_rgb8", src=f"{w}x{h}", dst=f"{nw}x{nh}")
        if not args.no_host:
            r = subprocess.run([SELFTEST, "resize-time", str(w), str(h), str(nw), str(nh)], capture_output=True, text=True,
                               timeout=args.step_timeout)
            if r.returncode != 0:
                sys.exit(f"host loop failed: {r.stderr}")
            row["host_ms"] = float(r.stdout.split()[0])
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
                            str(w), str(h), str(nw), str(nh), "--iters", str(args.iters), "--host-iters", str(args.host_iters)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"GPU step {w}x{h} -> {nw}x{nh} ended with status {r.returncode}; nothing more is run\n{r.stdout}{r.stderr}")
        row.update(json.loads(r.stdout.strip().splitlines()[-1]))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
