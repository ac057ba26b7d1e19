#!/usr/bin/env python3
"""Auto-exposure and tone mapping on one GPU: what the three kernels cost, and what the auto exposure does to the dimmed-light
sequence of the temporal-gradient section; one JSON line.
    python tools/tonemap_bench.py [--size 1024] [--reps 20] [--sequence] [--images DIR] [--baseline-only]

times: the film of C2 at --size (2 spp) on the device.  Between device events, medians over --reps calls after two untimed:
pt_film_histogram_device (memset + k_film_histogram), pt_tonemap_device in manual mode without / with the float plane
(k_tonemap alone) and in auto mode (memset, k_film_histogram, k_exposure_meter, k_tonemap); beside them pt_denoise_device with
iterations = 0 (k_denoise_init alone) and pt_film_pack (k_film_pack) on the same film.  Under `rocprofv3 --kernel-trace --stats`
the same calls give the per-kernel times.  --baseline-only: the two existing kernels alone (runs on a tree without the tone mapper).
--sequence: C2 at 128 x 128, 2 spp, 8 static frames, then the emission x 0.25 and 28 more, each frame through
pt_render_denoised_gradient; per frame the mean RGBA8 luminance with the fixed sqrt transform and with pt_tonemap_device at its
defaults, log2E, and the frames after the change until log2E is within 10 % of the step to its steady value.
--images DIR: frame 7, 8 and 35 of the sequence, fixed | auto side by side, as PPM files."""
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
    out = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out[2:]), 2)


def times(S, reps, baseline_only):
    dev = torch.device("cuda", 0)
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=S, height=S)
    prm = pt.default_params(spp=2)
    lin, rgba = ctx.render(cam, prm)
    feat = torch.from_numpy(ctx.render_features(cam, prm, 2)).to(dev)
    stream = torch.cuda.current_stream(dev)
    ctx.set_stream(stream.cuda_stream)
    out = torch.empty_like(lin)
    out8 = torch.empty_like(rgba)
    packed = torch.empty((S * S, 4), dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dn0 = pt.default_denoise(iterations=0)
    res = {"size": S, "unit": "us"}
    res["denoise_init"] = timed(lambda: check(lib().pt_denoise_device(ctx._h, S, S, P(lin), P(feat), C.byref(dn0), P(out), P(out8))), reps)
    res["film_pack"] = timed(lambda: check(lib().pt_film_pack(C.c_void_p(stream.cuda_stream or None), P(lin), P(rgba), S * S, P(packed))), reps)
    if not baseline_only:
        hist = torch.empty(258, dtype=torch.int32, device=dev)
        manual, auto = pt.default_tonemap(mode="manual"), pt.default_tonemap()
        res["histogram"] = timed(lambda: check(lib().pt_film_histogram_device(ctx._h, S, S, P(lin), P(hist))), reps)
        res["tonemap_manual_rgba"] = timed(lambda: check(lib().pt_tonemap_device(ctx._h, S, S, P(lin), C.byref(manual), None, P(out8))), reps)
        res["tonemap_manual_both"] = timed(lambda: check(lib().pt_tonemap_device(ctx._h, S, S, P(lin), C.byref(manual), P(out), P(out8))), reps)
        res["tonemap_auto_rgba"] = timed(lambda: check(lib().pt_tonemap_device(ctx._h, S, S, P(lin), C.byref(auto), None, P(out8))), reps)
        res["tonemap_auto_both"] = timed(lambda: check(lib().pt_tonemap_device(ctx._h, S, S, P(lin), C.byref(auto), P(out), P(out8))), reps)
        h = hist.cpu().numpy()
        res["bins_used"] = int((h[:256] > 0).sum())
        res["largest_bin_share"] = round(float(h.max() / h.sum()), 3)
    ctx.sync()
    ctx.close()
    return res


def luma8(rgba):
    return round(float((0.2126 * rgba[..., 0] + 0.7152 * rgba[..., 1] + 0.0722 * rgba[..., 2]).mean()), 2)


def write_ppm(path, left, right):
    img = np.concatenate([left[..., :3], right[..., :3]], axis=1)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def sequence(S, images):
    base = pt.builtin_scene(2)
    dim = (pt._lib.PtObject * len(base))(*base)
    for o in dim:
        if o.mat_tag == 1:
            for k in range(3):
                o.mat[k] *= 0.25
    cam = pt.camera_new(width=S, height=S)
    ctx = pt.Context(0)
    ctx.upload(base)
    N, change = 36, 8
    fixed, auto, log2E = [], [], []
    for i in range(N):
        if i == change:
            ctx.scene_update(dim)
        f = ctx.render_denoised_gradient(cam, pt.default_params(spp=2, spp_offset=2 * i), 2)
        rgba, _ = ctx.tonemap(f[0])
        fixed.append(luma8(f[1]))
        auto.append(luma8(rgba))
        log2E.append(round(ctx.exposure()[0], 4))
        if images and i in (change - 1, change, N - 1):
            os.makedirs(images, exist_ok=True)
            write_ppm(os.path.join(images, f"tonemap_frame{i:02d}_fixed_auto.ppm"), f[1], rgba)
    # the steady value: where the recursion is heading from the last frame, log2E + (t - log2E) with t from the last histogram
    before, last = log2E[change - 1], log2E[-1]
    steady = before + 2.0                                     # a quarter of the light: two octaves
    within = next((k + 1 for k, v in enumerate(log2E[change:]) if abs(v - steady) <= 0.1 * abs(steady - before)), None)
    ctx.close()
    return {"size": S, "frames": N, "change_at": change, "mean_luma8_fixed": fixed, "mean_luma8_auto": auto, "log2E": log2E,
            "log2E_last": last, "steady_log2E_expected": round(steady, 4), "frames_to_within_10pct": within,
            "frames_to_within_10pct_by_the_recursion": int(np.ceil(np.log(0.1) / np.log(1.0 - 0.1)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sequence", action="store_true")
    ap.add_argument("--images", default=None)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    res = {"times": times(args.size, args.reps, args.baseline_only)}
    if args.sequence or args.images:
        res["sequence"] = sequence(128, args.images)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
