#!/usr/bin/env python3
"""Times what a process pays before its first step: turning the checkpoint into the packed weight arena.  One JSON line per
context dtype (f16, bf16), four legs in one process, alternating, medians of --repeats (at least 10) with minimum and maximum:

  pt_host_ms       me_load_checkpoint_pt with the host packer (me_ctx_set_weight_packer 0): load_weight's loops on one core,
                   one synchronous pageable upload per tensor
  pt_device_ms     the same with the device packer (1): raw bytes through the pinned ring, one pack kernel per tensor
  cache_load_ms    me_load_weight_arena: the cache file through the pinned ring into the arena, checksum on the device
  cache_write_ms   me_save_weight_arena: checksum, the arena down through pinned memory, the parallel write, the rename
  legs_ms          me_last_weight_load beside each: stage (host wall clock), upload, pack, finalize (, cache_write)
  step_ms          one full-size me_extract_depth_u8 step of the same build (device pointers), for scale

The checkpoint is the full-size synthetic one (--config tiny for a dry run), written once as a torch.save file (f16) and
read once to warm the page cache: a cold disk measures the machine, not this code.  The device packer's arena and the
cache's are checked against the host packer's, byte for byte, before anything is timed.

    python3 tools/bench_checkpoint_load.py [--repeats 10] [--config full] [--dir DIR] [--out profiles/checkpoint_load_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--config", default="full", choices=("full", "tiny"))
    ap.add_argument("--dir", default=None, help="where the checkpoint and the cache files go (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats: at least 10")
    import torch
    import matrix_eyes_amd as m
    from matrix_eyes_amd.synthetic import synthetic_checkpoint, synthetic_images
    assert torch.cuda.is_available(), "bench_checkpoint_load needs a GPU"
    cfg = m.ModelConfig() if args.config == "full" else m.ModelConfig.tiny()
    work = args.dir or tempfile.mkdtemp(prefix="me_ckpt_")
    os.makedirs(work, exist_ok=True)
    ckpt = os.path.join(work, f"synthetic_{args.config}.pt")
    t0 = time.perf_counter()
    torch.save(synthetic_checkpoint(cfg), ckpt)
    with open(ckpt, "rb") as f:                      # warm the page cache
        while f.read(64 << 20):
            pass
    print(f"# checkpoint {ckpt}: {os.path.getsize(ckpt) / 1e6:.0f} MB, made in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    for dtype in ("f16", "bf16"):
        ctx = m.Context(0, dtype, cfg)
        cache = os.path.join(work, f"arena_{dtype}.mearena")

        def arena():
            ctx.synchronize()
            return ctx.weight_arena_tensor().clone()

        def pt_host():
            ctx.set_weight_packer("host")
            ctx.load_checkpoint_pt(ckpt)

        def pt_device():
            ctx.set_weight_packer("device")
            ctx.load_checkpoint_pt(ckpt)

        def cache_write():
            ctx.save_weight_arena(cache, ckpt)

        def cache_load():
            ctx.load_weight_arena(cache, ckpt)

        # warm-up and the check: pinned ring, events, the file's pages
        pt_host()
        want = arena()
        pt_device()
        assert torch.equal(arena(), want), "the device packer's arena differs from the host packer's"
        cache_write()
        cache_load()
        assert torch.equal(arena(), want), "the cache's arena differs from the host packer's"
        del want
        S = cfg.img_size
        rgb = torch.from_numpy(synthetic_images(1, S)).cuda()
        out = torch.empty(1, S, S, dtype=torch.float32, device="cuda")
        f_norm = torch.tensor([0.9], device="cuda")
        steps = []
        for i in range(13):
            ctx.synchronize()
            t = time.perf_counter()
            ctx.extract_depth(rgb, f_norm, out=out)
            ctx.synchronize()
            if i >= 3:
                steps.append((time.perf_counter() - t) * 1e3)
        times = {k: [] for k in ("pt_host", "pt_device", "cache_write", "cache_load")}
        legs = {k: [] for k in times}
        for r in range(args.repeats):
            for name, fn in (("pt_host", pt_host), ("pt_device", pt_device), ("cache_write", cache_write), ("cache_load", cache_load)):
                times[name].append(timed(fn))
                if name != "cache_write":
                    legs[name].append(ctx.last_weight_load()[1])
                else:
                    legs[name].append({"cache_write": ctx.last_weight_load()[1]["cache_write"]})
            print(f"# {dtype} repeat {r + 1}/{args.repeats}: " + ", ".join(f"{k} {v[-1]:.0f} ms" for k, v in times.items()),
                  file=sys.stderr, flush=True)
        rep = ctx.last_weight_load()[0]
        med = statistics.median
        row = dict(op="checkpoint_load", config=args.config, dtype=dtype, repeats=args.repeats,
                   checkpoint_bytes=os.path.getsize(ckpt), arena_bytes=ctx.weight_arena_bytes(), tensors=rep["tensors"],
                   step_ms=round(med(steps), 2))
        for k, v in times.items():
            row[f"{k}_ms"] = round(med(v), 1)
            row[f"{k}_ms_min"] = round(min(v), 1)
            row[f"{k}_ms_max"] = round(max(v), 1)
            row[f"{k}_legs_ms"] = {leg: round(med([x[leg] for x in legs[k]]), 2) for leg in legs[k][0]}
        row["device_vs_host"] = round(med(times["pt_host"]) / med(times["pt_device"]), 2)
        row["cache_vs_host"] = round(med(times["pt_host"]) / med(times["cache_load"]), 2)
        row["pt_host_steps"] = round(med(times["pt_host"]) / med(steps), 1)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        ctx.close()
        os.remove(cache)
    os.remove(ckpt)
    if not args.dir:
        os.rmdir(work)


if __name__ == "__main__":
    main()
