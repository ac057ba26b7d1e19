#!/usr/bin/env python3
"""Temporal denoiser on one GPU: a C2 camera fly-through at 1024^2, 1 spp and 1 feature sample per frame; one JSON line.
    python tools/temporal_bench.py [--frames N] [--size S] [--images DIR]
    python tools/temporal_bench.py --moving [--frames N] [--size S]

Per frame, on the context's stream between device events: render (pt_render_device), features
(pt_render_features_device), the temporal kernel and the a-trous steps (pt_denoise_temporal_device with iterations = 0,
and with the default 5 iterations; the steps are the difference), medians over the frames after the first.  fresh: the
fraction of fresh pixels per frame, read from a second pass over the same frames with a zero film followed by a film of
ones (a fresh pixel shows 1, a pixel with history 1 - alpha').  static_fresh: the same on frames of a camera that does not
move, with misses counted apart.  --images DIR writes noisy | spatial | temporal | 4096-spp reference of the last frame.

--moving: a static camera on C2 while the smallest sphere crosses the floor (pt_scene_update per frame).  The same film,
features and ids go to k_denoise_temporal_motion on one context and to k_denoise_temporal on a second one (iterations = 0: the
kernel alone, the motion entry's map upload included), device events, medians; then the motion kernel on a scene in which
nothing moves; then the host time of pt_scene_update against pt_scene_upload, alone and with the first 64 x 64 x 1 render
after it (which rebuilds the BVH where accel = 1), on C2 and on 10 000 spheres."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pathtrace_amd as pt  # noqa: E402
from pathtrace_amd._lib import check, lib  # noqa: E402


def fly(i, S):
    """frame i of the fly-through: an arc of 0.004 rad per frame around the box's centre, rising 0.01 per frame"""
    phi = 0.004 * i
    return pt.camera_look_at((4 * math.sin(phi), 0.01 * i, -2 + 4 * math.cos(phi)), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), S, S, 35.0)


def moving(args):
    import time
    dev = torch.device("cuda", 0)
    S, N = args.size, args.frames
    a, b = pt.Context(0), pt.Context(0)
    stream = torch.cuda.current_stream(dev)
    a.set_stream(stream.cuda_stream)
    b.set_stream(stream.cuda_stream)
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    feat = torch.empty((S, S, 8), dtype=torch.float32, device=dev)
    ids = torch.empty((S, S), dtype=torch.int32, device=dev)
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    base = pt.builtin_scene(2)
    ball = min((k for k, o in enumerate(base) if o.shape_tag == 0 and o.mat_tag != 1), key=lambda k: base[k].shape[3])
    cam = pt.camera_new(width=S, height=S)
    dn0, tp = pt.default_denoise(iterations=0), pt.default_temporal()

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def frame(i, move):
        objs = (pt._lib.PtObject * len(base))(*base)
        if move:
            objs[ball].shape[0] += 0.02 * (i - N // 2)
        a.scene_update(objs)
        p = pt.default_params(spp=1, spp_offset=i)
        check(lib().pt_render_device(a._h, C.byref(cam), C.byref(p), C.c_void_p(lin.data_ptr()), C.c_void_p(rgba.data_ptr())))
        check(lib().pt_render_features_device(a._h, C.byref(cam), C.byref(p), 1, C.c_void_p(feat.data_ptr())))
        check(lib().pt_render_feature_ids_device(a._h, C.byref(cam), C.byref(p), C.c_void_p(ids.data_ptr())))
        e0 = ev()
        check(lib().pt_denoise_temporal_motion_device(a._h, C.byref(cam), C.c_void_p(lin.data_ptr()), C.c_void_p(feat.data_ptr()),
                                                      C.c_void_p(ids.data_ptr()), C.byref(dn0), C.byref(tp), C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(rgba.data_ptr())))
        e1 = ev()
        check(lib().pt_denoise_temporal_device(b._h, C.byref(cam), C.c_void_p(lin.data_ptr()), C.c_void_p(feat.data_ptr()), C.byref(dn0),
                                               C.byref(tp), C.c_void_p(out.data_ptr()), C.c_void_p(rgba.data_ptr())))
        e2 = ev()
        e2.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    res = {"size": S, "frames": N}
    a.upload(base)
    for name, move in (("moving", True), ("standing", False)):
        a.temporal_reset()
        b.temporal_reset()
        t = [frame(i, move) for i in range(N)][1:]
        res[name + "_motion_kernel_ms"] = round(statistics.median(x[0] for x in t), 4)
        res[name + "_temporal_kernel_ms"] = round(statistics.median(x[1] for x in t), 4)
    small = pt.camera_new(width=64, height=64)
    for name, objs, accel in (("c2", base, 0), ("spheres_10000", pt.builtin_scene(4, 10000), 1)):
        p = pt.default_params(spp=1, accel=accel)
        a.upload(objs)
        a.render(small, p)
        for entry in ("upload", "update"):
            call, total = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                (a.upload if entry == "upload" else a.scene_update)(objs)
                t1 = time.perf_counter()
                a.render(small, p)
                a.sync()
                t2 = time.perf_counter()
                call.append((t1 - t0) * 1e3)
                total.append((t2 - t0) * 1e3)
            res[f"{name}_{entry}_ms"] = round(statistics.median(call), 3)
            res[f"{name}_{entry}_and_first_render_ms"] = round(statistics.median(total), 3)
    a.close()
    b.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--images", default=None)
    ap.add_argument("--moving", action="store_true", help="the motion entry against the existing one, and pt_scene_update against pt_scene_upload")
    args = ap.parse_args()
    if args.moving:
        return moving(args)
    dev = torch.device("cuda", 0)
    S, N = args.size, args.frames
    ctx = pt.Context(0)
    stream = torch.cuda.current_stream(dev)
    ctx.set_stream(stream.cuda_stream)
    h = ctx._h
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    feat = torch.empty((S, S, 8), dtype=torch.float32, device=dev)
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba2 = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    ctx.upload(pt.builtin_scene(2))
    dn5, dn0, tp = pt.default_denoise(), pt.default_denoise(iterations=0), pt.default_temporal()

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def temporal(cam, dn, src=lin):
        check(lib().pt_denoise_temporal_device(h, C.byref(cam), C.c_void_p(src.data_ptr()), C.c_void_p(feat.data_ptr()), C.byref(dn),
                                               C.byref(tp), C.c_void_p(out.data_ptr()), C.c_void_p(rgba2.data_ptr())))

    times = {k: [] for k in ("render", "features", "temporal_kernel", "temporal_total")}
    for i in range(N):
        cam = fly(i, S)
        p = pt.default_params(spp=1, spp_offset=i)
        e0 = ev()
        check(lib().pt_render_device(h, C.byref(cam), C.byref(p), C.c_void_p(lin.data_ptr()), C.c_void_p(rgba.data_ptr())))
        e1 = ev()
        check(lib().pt_render_features_device(h, C.byref(cam), C.byref(p), 1, C.c_void_p(feat.data_ptr())))
        e2 = ev()
        if i == 0:
            ctx.temporal_reset()
        temporal(cam, dn5)
        e3 = ev()
        e3.synchronize()
        if i:
            times["render"].append(e0.elapsed_time(e1))
            times["features"].append(e1.elapsed_time(e2))
            times["temporal_total"].append(e2.elapsed_time(e3))
    # the temporal kernel alone (iterations = 0 finalizes in it), on the same frames
    ctx.temporal_reset()
    for i in range(N):
        cam = fly(i, S)
        p = pt.default_params(spp=1, spp_offset=i)
        check(lib().pt_render_device(h, C.byref(cam), C.byref(p), C.c_void_p(lin.data_ptr()), C.c_void_p(rgba.data_ptr())))
        check(lib().pt_render_features_device(h, C.byref(cam), C.byref(p), 1, C.c_void_p(feat.data_ptr())))
        a = ev()
        temporal(cam, dn0)
        b = ev()
        b.synchronize()
        if i:
            times["temporal_kernel"].append(a.elapsed_time(b))
    res = {"size": S, "frames": N, "spp_per_frame": 1, "feature_samples": 1}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
    res["atrous_ms"] = round(res["temporal_total_ms"] - res["temporal_kernel_ms"], 4)

    def fresh_seq(cams):
        """per consecutive pair: frame i - 1 with a zero film, then frame i with ones, each with its own features"""
        zero = torch.zeros((S, S, 3), dtype=torch.float32, device=dev)
        ones = torch.ones((S, S, 3), dtype=torch.float32, device=dev)
        fr, miss = [], []
        for i in range(1, len(cams)):
            ctx.temporal_reset()
            p0, p1 = pt.default_params(spp=1, spp_offset=i - 1), pt.default_params(spp=1, spp_offset=i)
            check(lib().pt_render_features_device(h, C.byref(cams[i - 1]), C.byref(p0), 1, C.c_void_p(feat.data_ptr())))
            temporal(cams[i - 1], dn0, zero)
            check(lib().pt_render_features_device(h, C.byref(cams[i]), C.byref(p1), 1, C.c_void_p(feat.data_ptr())))
            temporal(cams[i], dn0, ones)
            o = out[..., 0].cpu().numpy()
            d = feat[..., 7].cpu().numpy()
            fr.append(round(float((o > 0.99).mean()), 5))
            miss.append(round(float((d == 0).mean()), 5))
        return fr, miss

    res["fresh"], res["miss"] = fresh_seq([fly(i, S) for i in range(min(N, 8))])
    res["static_fresh"], res["static_miss"] = fresh_seq([fly(0, S)] * 4)
    ctx.sync()
    if args.images:
        from PIL import Image
        ctx.temporal_reset()
        for i in range(N):
            t_lin, t8, noisy, _ = ctx.render_denoised_temporal(fly(i, S), pt.default_params(spp=1, spp_offset=i), 1)
        cam = fly(N - 1, S)
        _, s8, _, _ = ctx.render_denoised(cam, pt.default_params(spp=1, spp_offset=N - 1), 1)
        n8 = ctx.render(cam, pt.default_params(spp=1, spp_offset=N - 1))[1].cpu().numpy()
        r8 = ctx.render(cam, pt.default_params(spp=4096, spp_offset=1000000))[1].cpu().numpy()
        row = np.concatenate([n8[..., :3], s8[..., :3], t8[..., :3], r8[..., :3]], 1)
        os.makedirs(args.images, exist_ok=True)
        Image.fromarray(row).save(os.path.join(args.images, f"temporal_c2_{S}_1spp.png"), optimize=True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
