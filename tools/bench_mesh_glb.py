#!/usr/bin/env python3
"""Times me_output_mesh(".glb") -- the sections packed on the GPU -- against its one-thread host serialiser and against
me_output_mesh(".ply") for the same depth map and colours, one JSON line per scene (colour mode):

  glb_ms        the whole ".glb" call on the device path: mesh kernels, the bounds reduction and its read-back, the JSON
                built on the host, glb_format.hip's pack launch, one D2H copy into pinned memory, write_bytes_parallel.
                glb_mesh_ms / glb_format_ms / glb_d2h_ms / glb_file_ms: the four legs of me_last_mesh_timing; glb_bytes.
  ply_ms ...    the same call and legs for ".ply" (ply_format.hip), in the same process, alternating with the ".glb" calls
  glb_host_ms   the whole ".glb" call with ME_GLB_HOST_FORMAT=1 (the legs of a host serialiser are not reported): the
                switch is read once per process, so this arm is a child process with its own context on the same GPU
                that is asked for ONE call at a time -- the arms alternate and never use the GPU at the same moment
  file_ratio    glb_file_ms / ply_file_ms beside bytes_ratio = glb_bytes / ply_bytes: does the write shrink with the file?

All figures are medians over the same --repeats (at least 10) calls after 3 warm-up calls per arm; the minima and maxima
of the whole calls show the spread.  The .glb files of the two .glb arms are compared once per row.

    python3 tools/bench_mesh_glb.py [--repeats 10] [--size 1536] [--dir /tmp] [--out profiles/glb_format_ab.txt]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mesh_ply import scene_depth  # noqa: E402


class Arm:
    """one context, the scenes resident on its device; call() = one me_output_mesh in colour mode, wall clock in ms"""

    def __init__(self, n):
        import numpy as np
        import torch
        import matrix_eyes_amd as m
        self.n = n
        self.ctx = m.Context(0, "f16", m.ModelConfig.tiny())
        self.depth = {k: m.DeviceDepthMap(self.ctx, torch.from_numpy(scene_depth(n, k)).cuda(), (n, n)) for k in ("full", "scene")}
        self.pixels = torch.from_numpy(np.random.default_rng(6).integers(0, 256, size=(n, n, 3), dtype=np.uint8)).cuda()
        self.ctx.synchronize()

    def call(self, scene, path):
        d, n = self.depth[scene], self.n
        t0 = time.perf_counter()
        self.ctx._check(self.ctx.lib.me_output_mesh(self.ctx.handle, C.c_void_p(d.data.data_ptr()), n, n, n, n, path.encode(),
                                                    b"photo.jpg", 1, C.c_void_p(self.pixels.data_ptr())))
        return (time.perf_counter() - t0) * 1e3


def worker(n):
    """the host arm: `scene path` per line on stdin -> the call's ms on stdout"""
    arm = Arm(n)
    print("ready", flush=True)
    for line in sys.stdin:
        scene, path = line.split()
        print(repr(arm.call(scene, path)), flush=True)


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
    assert not {"ME_GLB_HOST_FORMAT", "ME_PLY_HOST_FORMAT"} & set(os.environ), "the parent times the device paths"
    import torch
    assert torch.cuda.is_available(), "bench_mesh_glb needs a GPU"
    n = args.size
    arm = Arm(n)
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--size", str(n)],
                             env=dict(os.environ, ME_GLB_HOST_FORMAT="1"), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert child.stdout.readline().strip() == "ready", "the host arm did not start"

        def host_call(scene, path):
            child.stdin.write(f"{scene} {path}\n")
            child.stdin.flush()
            return float(child.stdout.readline())

        with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
            glb_path, ply_path, host_path = (os.path.join(tmp, f) for f in ("device.glb", "device.ply", "host.glb"))
            for scene in ("full", "scene"):
                for _ in range(3):                                    # warm-up: buffers, pinned memory, page cache
                    arm.call(scene, glb_path)
                    arm.call(scene, ply_path)
                    host_call(scene, host_path)
                with open(glb_path, "rb") as a, open(host_path, "rb") as b:
                    assert a.read() == b.read(), "the two .glb arms wrote different files"
                glb, ply, host, glb_legs, ply_legs = [], [], [], [], []
                for _ in range(args.repeats):
                    glb.append(arm.call(scene, glb_path))
                    glb_legs.append(arm.ctx.last_mesh_timing())
                    ply.append(arm.call(scene, ply_path))
                    ply_legs.append(arm.ctx.last_mesh_timing())
                    host.append(host_call(scene, host_path))
                med = statistics.median
                row = dict(op="output_mesh_glb", scene=scene, mode="color", size=f"{n}x{n}", repeats=args.repeats)
                for name, whole, legs, path in (("glb", glb, glb_legs, glb_path), ("ply", ply, ply_legs, ply_path)):
                    assert legs[-1]["bytes"] == os.path.getsize(path)
                    row.update({f"{name}_bytes": legs[-1]["bytes"], f"{name}_ms": round(med(whole), 2),
                                f"{name}_ms_min": round(min(whole), 2), f"{name}_ms_max": round(max(whole), 2)})
                    for leg in ("mesh_ms", "format_ms", "d2h_ms", "file_ms"):
                        row[f"{name}_{leg}"] = round(med(t[leg] for t in legs), 3)
                row.update(glb_host_ms=round(med(host), 2), glb_host_ms_min=round(min(host), 2), glb_host_ms_max=round(max(host), 2),
                           glb_host_bytes=os.path.getsize(host_path), bytes_ratio=round(row["glb_bytes"] / row["ply_bytes"], 3),
                           file_ratio=round(row["glb_file_ms"] / row["ply_file_ms"], 3))
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
