#!/usr/bin/env python3
"""Feature-guided upsampling on one GPU: what the kernel and the one-call frame cost, and what the reconstruction costs in
error; one JSON line.
    python tools/upsample_bench.py [--size 1024] [--spp 16] [--reps 20] [--quality] [--sweep] [--images DIR]

times: C2 at --size, the low film at half the size.  Between device events, medians over --reps calls after two untimed:
pt_upsample_device (k_upsample) from the denoised low film, beside it pt_denoise_device with 5 iterations and with 0
(k_denoise_init + 5 k_denoise_step; k_denoise_init alone) and pt_render_features_device at full size, all on device planes;
then, between host clocks around the blocking calls, pt_render_denoised at full size and pt_render_denoised_upsampled from half
the size, --spp samples per traced pixel in both.  Under `rocprofv3 --kernel-trace --stats` the same calls give per-kernel times.
--quality: C2 and World::new() at --qsize (default 256) from half the size, relMSE (tests/denoise_ref.py rel_mse) against
--ref-spp samples at full size from sample 10^6, for (1) the full-size render at spp / 4, denoised -- the same number of paths
--, (2) the low render at spp, denoised, guided upsampling, (3) the same low film through plain bilinear upsampling (numpy).
--sweep: (2) over sigma_n x sigma_d around the defaults.
--images DIR: the low, bilinear and guided films of C2 side by side, as PPM files."""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pathtrace_amd as pt  # noqa: E402
from pathtrace_amd._lib import check, lib  # noqa: E402
import denoise_ref as dr  # noqa: E402
import upsample_ref as ur  # noqa: E402

SCENES = {"C2": 2, "World::new()": 1}


def timed(fn, reps):
    out = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out[2:]), 2)


def walled(fn, reps):
    out = []
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out[2:]), 3)


def times(S, spp, reps):
    dev = torch.device("cuda", 0)
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(2))
    s = S // 2
    cam, lo_cam = pt.camera_new(width=S, height=S), pt.camera_new(width=s, height=s)
    prm = pt.default_params(spp=spp)
    lo_lin, _, _, lo_feat = ctx.render_denoised(lo_cam, prm, 4)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_lo, d_lo_feat, d_feat = T(lo_lin), T(lo_feat), T(ctx.render_features(cam, prm, 4))
    d_full = ctx.render(cam, prm)[0]
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    out8 = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    feat2 = torch.empty((S, S, 8), dtype=torch.float32, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    up, dn5, dn0 = pt.default_upsample(), pt.default_denoise(), pt.default_denoise(iterations=0)
    res = {"size": S, "low": s, "spp": spp, "kernel_unit": "us", "frame_unit": "ms"}
    res["upsample"] = timed(lambda: check(lib().pt_upsample_device(ctx._h, s, s, P(d_lo), P(d_lo_feat), S, S, P(d_feat), C.byref(up), P(out), P(out8))), reps)
    res["upsample_no_rgba"] = timed(lambda: check(lib().pt_upsample_device(ctx._h, s, s, P(d_lo), P(d_lo_feat), S, S, P(d_feat), C.byref(up), P(out), None)), reps)
    res["denoise_5_full"] = timed(lambda: check(lib().pt_denoise_device(ctx._h, S, S, P(d_full), P(d_feat), C.byref(dn5), P(out), P(out8))), reps)
    res["denoise_0_full"] = timed(lambda: check(lib().pt_denoise_device(ctx._h, S, S, P(d_full), P(d_feat), C.byref(dn0), P(out), P(out8))), reps)
    res["denoise_5_low"] = timed(lambda: check(lib().pt_denoise_device(ctx._h, s, s, P(d_lo), P(d_lo_feat), C.byref(dn5), P(out), P(out8))), reps)
    res["features_4_full"] = timed(lambda: check(lib().pt_render_features_device(ctx._h, C.byref(cam), C.byref(prm), 4, P(feat2))), reps)
    res["features_4_low"] = timed(lambda: check(lib().pt_render_features_device(ctx._h, C.byref(lo_cam), C.byref(prm), 4, P(feat2))), reps)
    # bytes the kernel must move: 32 B in + 16 B out per pixel, and the low planes once (44 B per low pixel)
    res["upsample_min_bytes"] = 48 * S * S + 44 * s * s
    ctx.sync()
    res["render_denoised_full"] = walled(lambda: ctx.render_denoised(cam, prm, 4), max(3, reps // 4))
    res["render_denoised_upsampled"] = walled(lambda: ctx.render_denoised_upsampled(cam, prm, (s, s), 4), max(3, reps // 4))
    res["render_full"] = walled(lambda: (ctx.render(cam, prm), ctx.sync()), max(3, reps // 4))
    res["render_low"] = walled(lambda: (ctx.render(lo_cam, prm), ctx.sync()), max(3, reps // 4))
    ctx.close()
    return res


def to8(lin):
    return dr.rgba8(np.asarray(lin, np.float32))[..., :3]


def write_ppm(path, panels):
    img = np.concatenate(panels, axis=1)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def quality(S, spp, ref_spp, sweep, images):
    ctx = pt.Context(0)
    s = S // 2
    cam, lo_cam = pt.camera_new(width=S, height=S), pt.camera_new(width=s, height=s)
    res = {"size": S, "low": s, "spp_low": spp, "spp_full_equal_paths": max(1, spp // 4), "ref_spp": ref_spp}
    for name, scene in SCENES.items():
        ctx.upload(pt.builtin_scene(scene))
        ref = ctx.render(cam, pt.default_params(spp=ref_spp, spp_offset=1000000))[0].cpu().numpy().astype(np.float64)
        full = ctx.render_denoised(cam, pt.default_params(spp=max(1, spp // 4)), 4)
        guided, _, lo, feat = ctx.render_denoised_upsampled(cam, pt.default_params(spp=spp), (s, s), 4)
        plain = ur.bilinear(lo, S, S)
        r = {"full_spp4_denoised": dr.rel_mse(full[0], ref), "full_spp4_noisy": dr.rel_mse(full[2], ref),
             "low_guided": dr.rel_mse(guided, ref), "low_bilinear": dr.rel_mse(plain, ref)}
        # the same at equal spp: what the full-size frame of four times the paths reaches
        r["full_spp_denoised"] = dr.rel_mse(ctx.render_denoised(cam, pt.default_params(spp=spp), 4)[0], ref)
        if sweep:
            lo_feat = ctx.render_features(lo_cam, pt.default_params(spp=spp), 4)
            r["sweep"] = {f"{sn:g}/{sd:g}": round(dr.rel_mse(ctx.upsample(lo, lo_feat, feat, sigma_n=sn, sigma_d=sd)[0], ref), 6)
                          for sn in (32.0, 128.0, 512.0) for sd in (0.00625, 0.025, 0.1, 0.4)}
        res[name] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items()}
        if images and scene == 2:
            os.makedirs(images, exist_ok=True)
            nearest = np.repeat(np.repeat(lo, 2, axis=0), 2, axis=1)[:S, :S]
            write_ppm(os.path.join(images, "upsample_low_bilinear_guided.ppm"), [to8(nearest), to8(plain), to8(guided)])
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--qsize", type=int, default=256)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--images", default=None)
    args = ap.parse_args()
    res = {"times": times(args.size, args.spp, args.reps)}
    if args.quality or args.sweep or args.images:
        res["quality"] = quality(args.qsize, args.spp, args.ref_spp, args.sweep, args.images)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
