#!/usr/bin/env python3
"""The variance-guided filter after an adaptive render on one GPU; prints one JSON line.
    python tools/adaptive_denoise_bench.py [--reps N] [--size S] [--quality]

The job: C2, spp_min 4, spp_step 4, spp_max 64, rel_tol 0.05, 4 feature samples, pt_default_denoise (5 iterations).
Times at --size (1024), medians over --reps after one warm-up:
  device events around each call on the context's stream
    variance_ms            pt_adaptive_variance_device (k_adaptive_variance alone)
    denoise_{1,5}it_ms     pt_denoise_device: k_denoise_init + 1 or 5 k_denoise_step
    var_{1,5}it_*_ms       pt_denoise_var_device with the measured plane, an all-NaN plane (every lane falls back) and a
                           plane with every third pixel NaN; the steps are the same launches, so the difference to
                           denoise_*it_ms is k_denoise_init_var against k_denoise_init
  host clock around blocking calls
    one_call_ms            pt_render_adaptive_denoised
    two_calls_ms           pt_render_adaptive, then what pt_render_denoised runs behind its render: the film back to the
                           device, pt_render_features_device, pt_denoise_device, pt_sync, the film to the host
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
--quality adds relMSE over the non-emitter pixels at 128^2 against 4096 spp from sample 10^6, for C2 and World::new():
(a) the adaptive film, (b) pt_denoise_device on it, (c) pt_render_adaptive_denoised."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pathtrace_amd as pt  # noqa: E402
from pathtrace_amd._lib import PtAdaptive, check, lib  # noqa: E402

JOB = dict(spp_min=4, spp_step=4, rel_tol=0.05)


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


def host_timed(fn, reps):
    """median ms of the blocking fn() on the host clock (one warm-up call first)"""
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def rel_mse(x, ref):
    return float(np.mean((np.asarray(x, np.float64) - ref) ** 2 / (ref ** 2 + 0.01)))


def quality(ctx, scene):
    ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=128, height=128)
    prm = pt.default_params(spp=64)
    c_lin, _, noisy, spp, _, var = ctx.render_adaptive_denoised(cam, prm, feature_samples=4, iterations=5, **JOB)
    feat = ctx.render_features(cam, prm, 4)
    b_lin, _ = ctx.denoise(noisy, feat, iterations=5)
    ref = ctx.render(cam, pt.default_params(spp=4096, spp_offset=1000000))[0].cpu().numpy().astype(np.float64)
    m = feat[..., 3] == 0
    a, b, c = (rel_mse(x[m], ref[m]) for x in (noisy, b_lin, c_lin))
    return {"mean_spp": float(spp.mean()), "relmse_adaptive": a, "relmse_denoise": b, "relmse_denoise_var": c, "c_over_a": c / a,
            "c_over_b": c / b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--quality", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S = args.size
    ctx = pt.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h = ctx._h
    cam = pt.camera_new(width=S, height=S)
    prm = pt.default_params(spp=64)
    ad = PtAdaptive(JOB["spp_min"], JOB["spp_step"], JOB["rel_tol"], 1e-3)
    res = {"size": S, "reps": args.reps}
    ctx.upload(pt.builtin_scene(2))
    h_lin = np.empty((S, S, 3), np.float32)
    h_out = np.empty((S, S, 3), np.float32)
    h_spp = np.empty((S, S), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = lambda t: C.c_void_p(t.data_ptr())

    def adaptive():
        check(lib().pt_render_adaptive(h, C.byref(cam), C.byref(prm), C.byref(ad), p(h_lin), None, p(h_spp), None))

    adaptive()
    res["mean_spp"] = float(h_spp.mean())
    lin = torch.from_numpy(h_lin).to(dev)
    feat = torch.empty((S, S, 8), dtype=torch.float32, device=dev)
    var = torch.empty((S, S), dtype=torch.float32, device=dev)
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    check(lib().pt_render_features_device(h, C.byref(cam), C.byref(prm), 4, d(feat)))
    res["variance_ms"] = timed(lambda: check(lib().pt_adaptive_variance_device(h, S, S, d(feat), d(var))), args.reps)
    nan = torch.full_like(var, float("nan"))
    third = var.clone()
    third.view(-1)[::3] = float("nan")
    for it in (1, 5):
        dn = pt.default_denoise(iterations=it)
        res[f"denoise_{it}it_ms"] = timed(lambda: check(lib().pt_denoise_device(h, S, S, d(lin), d(feat), C.byref(dn), d(out), None)), args.reps)
        for name, plane in (("measured", var), ("nan", nan), ("third_nan", third)):
            res[f"var_{it}it_{name}_ms"] = timed(
                lambda: check(lib().pt_denoise_var_device(h, S, S, d(lin), d(feat), d(plane), C.byref(dn), d(out), None)), args.reps)
    dn = pt.default_denoise()

    def one_call():
        check(lib().pt_render_adaptive_denoised(h, C.byref(cam), C.byref(prm), C.byref(ad), 4, C.byref(dn), p(h_out), None, None, None, None,
                                                None))

    def two_calls():
        adaptive()
        lin.copy_(torch.from_numpy(h_lin))
        check(lib().pt_render_features_device(h, C.byref(cam), C.byref(prm), 4, d(feat)))
        check(lib().pt_denoise_device(h, S, S, d(lin), d(feat), C.byref(dn), d(out), None))
        ctx.sync()
        h_out[...] = out.cpu().numpy()

    res["adaptive_ms"] = host_timed(adaptive, args.reps)
    res["one_call_ms"] = host_timed(one_call, args.reps)
    res["two_calls_ms"] = host_timed(two_calls, args.reps)
    if args.quality:
        res["quality_c2"] = quality(ctx, 2)
        res["quality_world_new"] = quality(ctx, 1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
