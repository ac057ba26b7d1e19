#!/usr/bin/env python3
"""Times of the bloom stage on one GPU by HIP events (docs/EXPERIMENTS.md, "Bloom").
    python tools/bloom_bench.py [--size 1024] [--reps 200] [--images DIR]
Prints one JSON line: whole-call times of pt_bloom_device at size^2 for 1 .. 8 levels with the tail kernel and without it (the step
from one level count to the next is what that level's kernels cost), and pt_display_device beside pt_tonemap_device alone.
--images DIR: World::new() at 400 x 400, 64 spp, written as DIR/bloom_off.ppm and DIR/bloom_on.ppm (pt_display_device without and
with the default bloom, ACES)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtrace_amd as pt  # noqa: E402


def timed(fn, reps, torch):
    """median and minimum of `reps` single calls, each between two events, in microseconds"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(out)), 2), round(float(np.min(out)), 2)


def write_ppm(path, rgba):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgba.shape[1], rgba.shape[0]))
        f.write(np.ascontiguousarray(rgba[..., :3]).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--images")
    args = ap.parse_args()
    import torch
    lib, check = pt._lib.lib(), pt._lib.check
    ctx = pt.Context(0)
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    S = args.size
    rng = np.random.default_rng(0)
    film = np.exp2(rng.uniform(-8.0, 4.0, (S, S, 3))).astype(np.float32)
    d_in = torch.from_numpy(film).to(dev)
    d_out = torch.empty_like(d_in)
    d_rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    pin, pout, p8 = (C.c_void_p(t.data_ptr()) for t in (d_in, d_out, d_rgba))
    res = {"size": S, "reps": args.reps, "unit": "us (median, min)", "bloom": {}, "bloom_no_tail": {}}
    for tail in (True, False):
        ctx.bloom_tail(tail)
        for levels in range(1, 9):
            b = pt.default_bloom(levels=levels)
            res["bloom" if tail else "bloom_no_tail"][levels] = timed(lambda: check(lib.pt_bloom_device(ctx._h, S, S, pin, C.byref(b), pout)), args.reps, torch)
    ctx.bloom_tail(True)
    tm, b = pt.default_tonemap(), pt.default_bloom()
    res["tonemap"] = timed(lambda: check(lib.pt_tonemap_device(ctx._h, S, S, pin, C.byref(tm), pout, p8)), args.reps, torch)
    res["display"] = timed(lambda: check(lib.pt_display_device(ctx._h, S, S, pin, C.byref(b), C.byref(tm), pout, p8)), args.reps, torch)
    res["display_null_bloom"] = timed(lambda: check(lib.pt_display_device(ctx._h, S, S, pin, None, C.byref(tm), pout, p8)), args.reps, torch)
    if args.images:
        os.makedirs(args.images, exist_ok=True)
        ctx.upload(pt.builtin_scene(1))
        lin = ctx.render(pt.camera_new(width=400, height=400), pt.default_params(spp=64))[0].cpu().numpy()
        for name, bl in (("bloom_off", None), ("bloom_on", pt.default_bloom())):
            ctx.exposure_reset()
            write_ppm(os.path.join(args.images, name + ".ppm"), ctx.display(lin, bl, curve="aces")[0])
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
