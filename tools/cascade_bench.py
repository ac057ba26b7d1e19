#!/usr/bin/env python3
"""The brightness cascade (pt_render_cascade_device): quality and time; prints one JSON line.
    python tools/cascade_bench.py kappa   [--size 64] [--spp 16] [--ref-spp 4096] [--threads N]     (CPU only)
    python tools/cascade_bench.py quality [--size 128] [--spp 16] [--ref-spp 4096]                  (one GPU)
    python tools/cascade_bench.py time    [--size 1024] [--spp 64] [--reps 9]                       (one GPU)

kappa    the choice of pt_default_cascade's kappa, without a GPU: per-sample radiance of World::new() from the f32 oracle, the
         rule on the CPU (pt_cascade_host) for kappa in {1, 2, 4, 8}, against an oracle reference from sample 10^6.  Per kappa:
         plain MSE, relMSE and the ratio of the film's mean to the reference's.
quality  World::new() and C2: the plain film and the cascade film of one render against a reference of --ref-spp samples from
         sample 10^6, and both through pt_denoise_device (4 feature samples, pt_default_denoise).
time     device events around each call on the context's stream, medians over --reps after one warm-up: pt_render_device and
         pt_render_cascade_device on C2, and the two cascade kernels alone on the samples of a render (pt_cascade_samples_device).
         Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this mode."""
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

KAPPAS = (1.0, 2.0, 4.0, 8.0)


def mse(x, ref):
    return float(np.mean((np.asarray(x, np.float64) - ref) ** 2))


def rel_mse(x, ref):
    """mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01): the denoiser's figure"""
    return float(np.mean((np.asarray(x, np.float64) - ref) ** 2 / (ref ** 2 + 0.01)))


def figures(x, ref):
    return {"mse": mse(x, ref), "rel_mse": rel_mse(x, ref), "mean_ratio": float(np.mean(x, dtype=np.float64) / ref.mean())}


def mode_kappa(args):
    from oracle import orc
    S = args.size
    objs = pt.builtin_scene(1)
    cam = pt.camera_new(width=S, height=S)
    xy = np.array([(x, y) for y in range(S) for x in range(S)], dtype=np.uint32)
    _, smp = orc.render_pixels(cam, objs, pt.default_params(spp=args.spp), xy, orc.F32, orc.ITERATIVE)
    samples = np.ascontiguousarray(smp.reshape(S, S, args.spp, 3).transpose(2, 0, 1, 3), dtype=np.float32)
    ref, _, _ = orc.render(cam, objs, pt.default_params(spp=args.ref_spp, spp_offset=1000000), orc.F32, orc.ITERATIVE, threads=args.threads)
    res = {"mode": "kappa", "size": S, "spp": args.spp, "ref_spp": args.ref_spp}
    plain = None
    for kappa in KAPPAS:
        film, _, plain, _, _ = pt.cascade_host(samples, pt.default_cascade(kappa=kappa))
        res["kappa_%g" % kappa] = figures(film, ref)
    res["plain"] = figures(plain, ref)
    return res


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


def mode_quality(args):
    S = args.size
    ctx = pt.Context(0)
    cam = pt.camera_new(width=S, height=S)
    res = {"mode": "quality", "size": S, "spp": args.spp, "ref_spp": args.ref_spp, "kappa": pt.default_cascade().kappa}
    for name, scene in (("world_new", 1), ("c2", 2)):
        ctx.upload(pt.builtin_scene(scene))
        prm = pt.default_params(spp=args.spp)
        ref = ctx.render(cam, pt.default_params(spp=args.ref_spp, spp_offset=1000000))[0].cpu().numpy().astype(np.float64)
        film, _, plain, _, _ = ctx.render_cascade(cam, prm)
        feat = ctx.render_features(cam, prm, 4)
        feat = feat.cpu().numpy() if hasattr(feat, "cpu") else feat
        res[name] = {"plain": figures(plain, ref), "cascade": figures(film, ref),
                     "plain_denoised": figures(ctx.denoise(plain, feat)[0], ref), "cascade_denoised": figures(ctx.denoise(film, feat)[0], ref)}
    ctx.close()
    return res


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
    for K in (2, 6, 8):
        cs = pt.default_cascade(layers=K)
        res["render_cascade_K%d_ms" % K] = timed(
            lambda: check(lib().pt_render_cascade_device(h, C.byref(cam), C.byref(prm), C.byref(cs), ptr(lin), ptr(rgba), ptr(plain))), args.reps)
    # the two kernels alone, on samples of the film's magnitude (the film itself, repeated: the kernels' time does not depend on
    # the values beyond which layers they reach)
    n = min(args.spp, 16)
    smp = lin.unsqueeze(0).repeat(n, 1, 1, 1).contiguous()
    for K in (2, 6, 8):
        cs = pt.default_cascade(layers=K)
        res["cascade_samples_n%d_K%d_ms" % (n, K)] = timed(
            lambda: check(lib().pt_cascade_samples_device(h, C.byref(cs), S, S, n, 0, ptr(smp), ptr(lin), ptr(rgba), ptr(plain))), args.reps)
    ctx.sync()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kappa", "quality", "time"))
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    args.size = args.size or {"kappa": 64, "quality": 128, "time": 1024}[args.mode]
    args.spp = args.spp or (64 if args.mode == "time" else 16)
    print(json.dumps({"kappa": mode_kappa, "quality": mode_quality, "time": mode_time}[args.mode](args)))


if __name__ == "__main__":
    main()
