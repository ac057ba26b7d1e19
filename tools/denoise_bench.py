#!/usr/bin/env python3
"""First-hit features and the a-trous denoiser on one GPU at 1024^2; prints one JSON line.
    python tools/denoise_bench.py [--reps N] [--size S] [--images DIR]

Times (device events around each call on the context's stream, medians over --reps after one warm-up):
  render_16 / render_64   pt_render_device of C2 at 16 and 64 spp (the job the filter serves)
  features_c2             pt_render_features_device, 4 samples, C2 (scan in LDS)
  features_c4_bvh         the same on C4 (10 000 spheres) with accel = BVH
  denoise                 pt_denoise_device, pt_default_denoise (5 iterations)
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
--images DIR writes World::new() at 256^2: 16 spp noisy | denoised | 4096 spp reference, side by side, as one PNG."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pathtrace_amd as pt  # noqa: E402
from pathtrace_amd._lib import check, lib  # noqa: E402


def timed(fn, reps):
    """median ms of fn() between two events on the current stream (one warm-up call first)"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--images", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S = args.size
    ctx = pt.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h = ctx._h
    cam = pt.camera_new(width=S, height=S)
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    feat = torch.empty((S, S, 8), dtype=torch.float32, device=dev)
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba2 = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    res = {"size": S, "reps": args.reps}

    def render(spp):
        p = pt.default_params(spp=spp)
        return lambda: check(lib().pt_render_device(h, C.byref(cam), C.byref(p), C.c_void_p(lin.data_ptr()), C.c_void_p(rgba.data_ptr())))

    def features(accel):
        p = pt.default_params(spp=16, accel=accel)
        return lambda: check(lib().pt_render_features_device(h, C.byref(cam), C.byref(p), 4, C.c_void_p(feat.data_ptr())))

    dn = pt.default_denoise()

    def denoise():
        check(lib().pt_denoise_device(h, S, S, C.c_void_p(lin.data_ptr()), C.c_void_p(feat.data_ptr()), C.byref(dn),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(rgba2.data_ptr())))

    ctx.upload(pt.builtin_scene(2))
    res["render_16_ms"] = timed(render(16), args.reps)
    res["render_64_ms"] = timed(render(64), args.reps)
    res["features_c2_ms"] = timed(features(0), args.reps)
    res["denoise_ms"] = timed(denoise, args.reps)
    ctx.upload(pt.builtin_scene(4, 10000))
    res["features_c4_bvh_ms"] = timed(features(1), args.reps)
    ctx.sync()
    if args.images:
        from PIL import Image
        ctx.upload(pt.builtin_scene(1))
        c256 = pt.camera_new(width=256, height=256)
        _, d8, _, _ = ctx.render_denoised(c256, pt.default_params(spp=16), 4)
        n8 = ctx.render(c256, pt.default_params(spp=16))[1].cpu().numpy()
        r8 = ctx.render(c256, pt.default_params(spp=4096, spp_offset=1000000))[1].cpu().numpy()
        row = np.concatenate([n8[..., :3], d8[..., :3], r8[..., :3]], 1)
        os.makedirs(args.images, exist_ok=True)
        Image.fromarray(row).save(os.path.join(args.images, "denoise_cornell_256_16spp.png"), optimize=True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
