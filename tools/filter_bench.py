#!/usr/bin/env python3
"""The film's reconstruction filters (pt_render_filtered_device): time and quality; prints one JSON line.
    python tools/filter_bench.py time    [--size 1024] [--spp 64] [--reps 9]                       (one GPU)
    python tools/filter_bench.py quality [--size 128] [--spp 16] [--ref-spp 4096]                  (one GPU)

time     device events around each call on the context's stream, medians over --reps after one warm-up: pt_render_device and
         pt_render_filtered_device on C2 for box 0.5 (M = 0), tent 1 and Gaussian 1.5 (M = 1), Gaussian 2.5 and Mitchell 2 (M = 2),
         and k_resolve_filter alone on 16 samples of the film's magnitude (pt_filter_samples_device).  Per-kernel times come
         from a separate `rocprofv3 --kernel-trace --stats` run of this mode.
quality  World::new(): for each of box 0.5, tent 1, Gaussian 1.5 (alpha 2) and Mitchell 2 (1/3, 1/3) the relMSE of the --spp film
         against a film of --ref-spp samples from sample 10^6 resolved WITH THE SAME FILTER (what the filter converges to), and
         against the box reference."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pathtrace_amd as pt  # noqa: E402
from pathtrace_amd._lib import check, lib  # noqa: E402

FILTERS = (("box_0.5", dict(kind="box", radius=0.5)), ("tent_1", dict(kind="tent", radius=1.0)),
           ("gaussian_1.5_2", dict(kind="gaussian", radius=1.5, a=2.0)), ("gaussian_2.5_2", dict(kind="gaussian", radius=2.5, a=2.0)),
           ("mitchell_2", dict(kind="mitchell", radius=2.0, a=1.0 / 3.0, b=1.0 / 3.0)))


def rel_mse(x, ref):
    """mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01): the denoiser's figure"""
    return float(np.mean((np.asarray(x, np.float64) - ref) ** 2 / (ref ** 2 + 0.01)))


def timed(fn, reps):
    """median ms of fn() between two events on the current stream (one warm-up call first)"""
    import torch
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


def mode_time(args):
    import torch
    dev = torch.device("cuda", 0)
    S = args.size
    ctx = pt.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h = ctx._h
    cam = pt.camera_new(width=S, height=S)
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    plain = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    prm = pt.default_params(spp=args.spp)
    res = {"mode": "time", "size": S, "spp": args.spp, "reps": args.reps}
    ctx.upload(pt.builtin_scene(2))
    res["render_ms"] = timed(lambda: check(lib().pt_render_device(h, C.byref(cam), C.byref(prm), ptr(lin), ptr(rgba))), args.reps)
    for name, over in FILTERS:
        flt = pt.default_filter(**over)
        res["render_filtered_%s_ms" % name] = timed(
            lambda: check(lib().pt_render_filtered_device(h, C.byref(cam), C.byref(prm), C.byref(flt), ptr(lin), ptr(rgba), ptr(plain))), args.reps)
    res["render_again_ms"] = timed(lambda: check(lib().pt_render_device(h, C.byref(cam), C.byref(prm), ptr(lin), ptr(rgba))), args.reps)
    # the kernel alone, on samples of the film's magnitude (the film itself, repeated: its time does not depend on the values)
    n = min(args.spp, 16)
    check(lib().pt_render_device(h, C.byref(cam), C.byref(prm), ptr(lin), ptr(rgba)))
    smp = lin.unsqueeze(0).repeat(n, 1, 1, 1).contiguous()
    out = torch.empty_like(lin)
    for name, over in FILTERS:
        flt = pt.default_filter(**over)
        res["filter_samples_n%d_%s_ms" % (n, name)] = timed(
            lambda: check(lib().pt_filter_samples_device(h, C.byref(flt), S, S, n, 0, 0, ptr(smp), ptr(out), ptr(rgba), ptr(plain), None)), args.reps)
    ctx.sync()
    ctx.close()
    return res


def mode_quality(args):
    S = args.size
    ctx = pt.Context(0)
    cam = pt.camera_new(width=S, height=S)
    ctx.upload(pt.builtin_scene(1))
    prm, ref_prm = pt.default_params(spp=args.spp), pt.default_params(spp=args.ref_spp, spp_offset=1000000)
    res = {"mode": "quality", "scene": "world_new", "size": S, "spp": args.spp, "ref_spp": args.ref_spp}
    box_ref = None
    for name, over in FILTERS[:3] + FILTERS[4:]:
        flt = pt.default_filter(**over)
        ref = ctx.render_filtered(cam, ref_prm, flt)[0].astype(np.float64)
        box_ref = ref if box_ref is None else box_ref
        film = ctx.render_filtered(cam, prm, flt)[0]
        res[name] = {"rel_mse_same_filter": rel_mse(film, ref), "rel_mse_box_reference": rel_mse(film, box_ref),
                     "reference_vs_box_reference": rel_mse(ref, box_ref), "min": float(film.min())}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "quality"))
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    args.size = args.size or {"quality": 128, "time": 1024}[args.mode]
    args.spp = args.spp or (64 if args.mode == "time" else 16)
    print(json.dumps({"quality": mode_quality, "time": mode_time}[args.mode](args)))


if __name__ == "__main__":
    main()
