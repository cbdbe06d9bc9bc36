#!/usr/bin/env python3
"""Times the four ways a stereogram can get its noise, one JSON line per picture size.  The depth map
(1536 x 1536, tests/png_pictures.py) is already on the device and the picture stays there; amplitude 1/16.

  a  legacy     std::mt19937 fills out_h * out_w * 3 bytes on one core, then me_stereogram from that HOST pointer.  The fill is
                the host layer's loop (host/matrix_eyes.cpp output_stereogram) compiled into the library
                (me_op_legacy_noise_host) so that it runs in this process: not the host layer's own object code.
  b  host twin  me_stereogram_noise_host (ChaCha12 on one core), then the same call
  c  fill       me_stereogram_noise into DEVICE memory, then me_stereogram from that device pointer: two launches
  d  keyed      me_stereogram_keyed: leg c's two launches behind one entry, the noise in context scratch (the first part of
                profiles/stereogram_noise_ab.txt was measured when a fused kernel stood here; it did not beat c and was deleted)

Per leg: gen_ms (the generation: wall clock on the host for a and b, wall clock with a device synchronise for c, 0 for d),
call_ms (the stereogram call, wall clock with a device synchronise; for a and b it holds the upload from pageable memory),
upload_ms (a, b: call_ms minus the kernel-only call of leg c, a derived figure), kernel_ms (HIP event time of the
fill kernel, me_last_stereogram_noise, in c and d) and total_ms = gen_ms + call_ms.  Medians of
--repeats (at least 10) after a warm-up, the four legs alternating in one process; *_min / *_max are the spread of the totals.

    python3 tools/bench_stereogram_noise.py [--repeats 10] [--sizes 1536x1536,4032x3024] [--out profiles/stereogram_noise_ab.txt]
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
    ap.add_argument("--sizes", default="1536x1536,4032x3024")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    import numpy as np
    import torch
    import matrix_eyes_amd as m
    import png_pictures as pic
    assert torch.cuda.is_available(), "bench_stereogram_noise needs a GPU"
    ctx = m.Context(0, "f16", m.ModelConfig.tiny())
    lib, h = ctx.lib, ctx.handle
    amp = 1.0 / 16.0
    dm = m.DepthMap(ctx, pic.inverse_depth_field(1536), (1536, 1536))
    mn, mx = dm.inverse_depth_range()
    depth = torch.from_numpy(dm.data).cuda()
    rows, cols = dm.data.shape
    key = (C.c_uint8 * 32)()
    lib.me_noise_key_from_seed(7, key)

    def vp(a):
        return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def last_noise():
        report, ms = (C.c_int64 * 2)(), C.c_double()
        ctx._check(lib.me_last_stereogram_noise(h, report, C.byref(ms)))
        return report[0], report[1], ms.value

    lines = []
    for size in args.sizes.split(","):
        w, hh = (int(v) for v in size.split("x"))
        nbytes = w * hh * 3
        noise_host = np.empty((hh, w, 3), np.uint8)
        noise_dev = torch.empty((hh, w, 3), dtype=torch.uint8, device="cuda")
        out = torch.empty((hh, w, 3), dtype=torch.uint8, device="cuda")

        def stereo(noise):
            ctx._check(lib.me_stereogram(h, vp(depth), rows, cols, mn, mx, w, hh, amp, vp(noise), vp(out)))

        legs = {
            "a_legacy": (lambda: lib.me_op_legacy_noise_host(7, nbytes, vp(noise_host)), lambda: stereo(noise_host)),
            "b_host_twin": (lambda: ctx._check(lib.me_stereogram_noise_host(key, w, hh, vp(noise_host))), lambda: stereo(noise_host)),
            "c_fill": (lambda: ctx._check(lib.me_stereogram_noise(h, key, w, hh, vp(noise_dev))), lambda: stereo(noise_dev)),
            "d_keyed": (None, lambda: ctx._check(lib.me_stereogram_keyed(h, vp(depth), rows, cols, mn, mx, w, hh, amp, key, vp(out)))),
        }
        t = {name: {"gen": [], "call": [], "kernel": [], "total": []} for name in legs}
        words, pictures = {}, {}
        for rep in range(-2, args.repeats):          # two warm-up rounds
            for name, (gen, call) in legs.items():
                g = wall(gen) if gen else 0.0
                k = last_noise() if name == "c_fill" else None
                c = wall(call)
                k = last_noise() if name == "d_keyed" else k
                if rep < 0:
                    pictures[name] = out.cpu().numpy().copy()
                    continue
                t[name]["gen"].append(g), t[name]["call"].append(c), t[name]["total"].append(g + c)
                if k:
                    t[name]["kernel"].append(k[2])
                    words[name] = k[1]
        # b, c and d show one picture: the same key
        assert np.array_equal(pictures["b_host_twin"], pictures["c_fill"]) and np.array_equal(pictures["c_fill"], pictures["d_keyed"])
        med = statistics.median
        kernel_only = med(t["c_fill"]["call"])
        line = {"op": "stereogram_noise", "size": size, "amplitude": amp, "noise_bytes": nbytes, "repeats": args.repeats,
                "legacy_fill": "me_op_legacy_noise_host: the host layer's mt19937 loop compiled into the library, same process"}
        for name in legs:
            r = {"gen_ms": round(med(t[name]["gen"]), 3), "call_ms": round(med(t[name]["call"]), 3),
                 "total_ms": round(med(t[name]["total"]), 3), "total_ms_min": round(min(t[name]["total"]), 3),
                 "total_ms_max": round(max(t[name]["total"]), 3)}
            if name in ("a_legacy", "b_host_twin"):
                r["upload_ms"] = round(r["call_ms"] - kernel_only, 3)
            if t[name]["kernel"]:
                r["kernel_ms"] = round(med(t[name]["kernel"]), 3)
                r["noise_words"] = words[name]
            line[name] = r
        c, d = line["c_fill"], line["d_keyed"]
        spread_c = round(c["total_ms_max"] - c["total_ms_min"], 3)
        line["d_vs_c"] = {"c_minus_d_ms": round(c["total_ms"] - d["total_ms"], 3), "spread_of_c_ms": spread_c,
                          "d_beats_c_by_more_than_the_spread": c["total_ms"] - d["total_ms"] > spread_c}
        line["speedup_d_over_a"] = round(line["a_legacy"]["total_ms"] / d["total_ms"], 1)
        text = json.dumps(line)
        print(text, flush=True)
        lines.append(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
