#!/usr/bin/env python3
"""Times me_output_mesh(".ply") with the records packed on the GPU against the host serialiser it replaces, one JSON
line per (scene, vertex mode):

  host_ms      the whole call with ME_PLY_HOST_FORMAT=1: mesh kernels, the arrays copied to pageable host memory, every
               record serialised by one thread, buffered fwrite.  The switch is read once per process, so this arm runs
               in a child process that holds its own context on the same GPU and is asked for ONE call at a time:
               the two arms alternate, and never use the GPU at the same moment.
  device_ms    the whole call on the device path: mesh kernels, ply_format.hip, one D2H copy into pinned memory,
               write_bytes_parallel (file_write.hip).  mesh_ms / format_ms / d2h_ms / file_ms: the four legs of me_last_mesh_timing
               (medians over the same calls).
  copy_ms      a plain device-to-device copy of `bytes` bytes, wall clock around the copy and a synchronise like
               format_ms: what the packing kernel would cost if it only moved the file's bytes
  speedup      host_ms / device_ms

Scenes at 1536 x 1536, depth and colours resident on the device: "full" (a flat map: every vertex, every face) and
"scene" (the smooth background with nearer rectangles of the output tests).  3 warm-up and --repeats (at least 10)
timed calls per arm; the files of both arms are compared once per row.

    python3 tools/bench_mesh_ply.py [--repeats 10] [--size 1536] [--dir /tmp] [--out profiles/ply_format_ab.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = {"plain": 0, "color": 1}


def scene_depth(n, kind):
    import numpy as np
    if kind == "full":
        return np.full((n, n), 0.7, np.float32)
    rng = np.random.default_rng(n + 2)
    yy, xx = np.meshgrid(np.linspace(0, 1, n, dtype=np.float32), np.linspace(0, 1, n, dtype=np.float32), indexing="ij")
    d = 0.2 + 0.15 * np.sin(3 * xx + 2 * yy) + 0.1 * yy
    for _ in range(6):
        x0, y0 = rng.integers(0, n - n // 4, size=2)
        w, h = rng.integers(n // 16, n // 4, size=2)
        d[y0:y0 + h, x0:x0 + w] += rng.uniform(0.2, 1.5)
    d += rng.normal(0, 0.002, size=d.shape).astype(np.float32)
    return np.ascontiguousarray(d.astype(np.float32))


class Arm:
    """one context, the scenes resident on its device; call() = one me_output_mesh, wall clock in ms"""

    def __init__(self, n):
        import numpy as np
        import torch
        import matrix_eyes_amd as m
        self.m, self.torch, self.n = m, torch, n
        self.ctx = m.Context(0, "f16", m.ModelConfig.tiny())
        self.depth = {k: m.DeviceDepthMap(self.ctx, torch.from_numpy(scene_depth(n, k)).cuda(), (n, n)) for k in ("full", "scene")}
        self.pixels = torch.from_numpy(np.random.default_rng(6).integers(0, 256, size=(n, n, 3), dtype=np.uint8)).cuda()
        self.ctx.synchronize()

    def call(self, scene, mode, path):
        d, n = self.depth[scene], self.n
        t0 = time.perf_counter()
        self.ctx._check(self.ctx.lib.me_output_mesh(
            self.ctx.handle, C.c_void_p(d.data.data_ptr()), n, n, n, n, path.encode(), b"photo.jpg", MODES[mode],
            C.c_void_p(self.pixels.data_ptr()) if mode == "color" else None))
        return (time.perf_counter() - t0) * 1e3


def worker(n):
    """the host arm: `scene mode path` per line on stdin -> the call's ms on stdout"""
    arm = Arm(n)
    print("ready", flush=True)
    for line in sys.stdin:
        scene, mode, path = line.split()
        print(repr(arm.call(scene, mode, path)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--size", type=int, default=1536)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.size)
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    assert "ME_PLY_HOST_FORMAT" not in os.environ, "the parent times the device path"
    import torch
    assert torch.cuda.is_available(), "bench_mesh_ply needs a GPU"
    n = args.size
    arm = Arm(n)
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--size", str(n)],
                             env=dict(os.environ, ME_PLY_HOST_FORMAT="1"), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert child.stdout.readline().strip() == "ready", "the host arm did not start"

        def host_call(scene, mode, path):
            child.stdin.write(f"{scene} {mode} {path}\n")
            child.stdin.flush()
            return float(child.stdout.readline())

        with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
            dev_path, host_path = os.path.join(tmp, "device.ply"), os.path.join(tmp, "host.ply")
            for scene in ("full", "scene"):
                for mode in ("plain", "color"):
                    for _ in range(3):                                    # warm-up: buffers, pinned memory, page cache
                        arm.call(scene, mode, dev_path)
                        host_call(scene, mode, host_path)
                    with open(dev_path, "rb") as a, open(host_path, "rb") as b:
                        assert a.read() == b.read(), "the two arms wrote different files"
                    dev, host, legs = [], [], []
                    for _ in range(args.repeats):
                        dev.append(arm.call(scene, mode, dev_path))
                        legs.append(arm.ctx.last_mesh_timing())
                        host.append(host_call(scene, mode, host_path))
                    nbytes = legs[-1]["bytes"]
                    assert nbytes == os.path.getsize(dev_path)
                    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                    dst = torch.empty_like(src)
                    copy = []
                    for k in range(3 + args.repeats):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        dst.copy_(src)
                        torch.cuda.synchronize()
                        if k >= 3:
                            copy.append((time.perf_counter() - t0) * 1e3)
                    del src, dst
                    med = statistics.median
                    row = dict(op="output_mesh_ply", scene=scene, mode=mode, size=f"{n}x{n}", bytes=nbytes,
                               host_ms=round(med(host), 2), host_ms_min=round(min(host), 2), host_ms_max=round(max(host), 2),
                               device_ms=round(med(dev), 2), device_ms_min=round(min(dev), 2), device_ms_max=round(max(dev), 2),
                               mesh_ms=round(med(t["mesh_ms"] for t in legs), 3), format_ms=round(med(t["format_ms"] for t in legs), 3),
                               d2h_ms=round(med(t["d2h_ms"] for t in legs), 3), file_ms=round(med(t["file_ms"] for t in legs), 3),
                               copy_ms=round(med(copy), 3), speedup=round(med(host) / med(dev), 2), repeats=args.repeats)
                    line = json.dumps(row)
                    print(line, flush=True)
                    if args.out:
                        with open(args.out, "a") as f:
                            f.write(line + "\n")
    finally:
        child.stdin.close()
        child.wait(timeout=60)


if __name__ == "__main__":
    main()
