#!/usr/bin/env python3
"""Temporal gradients on one GPU: what pt_render_denoised_gradient costs beside pt_render_denoised_motion, and what it buys
when the lighting changes; one JSON line.
    python tools/gradient_bench.py [--frames N] [--sizes 128,1024] [--quality-size 128] [--skip-quality]

cost: C2 and World::new(), static, 2 spp and 2 feature samples per frame, per size.  The two calls alternate frame by frame
in one process, each on a context of its own; wall time of the blocking call, medians over the frames after the second.
gradient_entry_ms: pt_temporal_gradient_device between device events (its three kernels and the list render of 1/9 of the
frame's samples); alpha_kernel_ms / motion_kernel_ms: pt_denoise_temporal_alpha_device and the motion entry with
iterations = 0 (one kernel each) on the same buffers.

quality: relMSE per frame against a 1024-spp reference of the frame's scene (samples from 10^6), non-emitter pixels, for
both calls on (a) "moving": C2, the smallest sphere crosses the floor by 0.02 per frame (the sequence of
tools/temporal_bench.py --moving) and (b) "dimmed": C2, eight static frames, then every emission x 0.25 and twelve more.
frames_to_steady: frames after the change until relMSE is back within 1.25 x the median of the four frames before it.

    python tools/gradient_bench.py --camera [--size 1024] [--paths fixed,orbit] [--quality-size 128] [--skip-quality]
--camera: the moving-camera entry (pt_render_denoised_gradient_camera).  cost: C2 at --size, static scene, 2 spp; per path a
context of its own: "existing" pt_render_denoised_gradient and "fixed" the new entry under one camera, "orbit" the new entry
under the orbit of examples/gradient_frames.cpp --camera (one step per frame, so k_gradient_alpha_camera solves the
reprojection).  A round is three frames of every path, the paths alternating frame by frame; one untimed round, then seven
timed: wall ms per frame as median [min, max] of the rounds.  --paths limits the new entry's paths (a kernel trace of
--paths orbit holds only reprojecting dispatches of k_gradient_alpha_camera).  quality: C2, the orbit, the light dimmed to a
quarter from frame 8 of 20: relMSE per frame (non-emitter pixels, against 1024 spp through the frame's camera) of the motion
entry, the existing gradient entry and the new one."""
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
from pathtrace_amd._lib import check, lib  # noqa: E402


def copy(objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def cost(scene, S, N):
    dev = torch.device("cuda", 0)
    a, b = pt.Context(0), pt.Context(0)
    objs = pt.builtin_scene(scene)
    cam = pt.camera_new(width=S, height=S)
    for c in (a, b):
        c.upload(objs)
    tg, tm = [], []
    for i in range(N):
        p = pt.default_params(spp=2, spp_offset=2 * i)
        t0 = time.perf_counter()
        a.render_denoised_gradient(cam, p, 2)
        t1 = time.perf_counter()
        b.render_denoised_motion(cam, p, 2)
        t2 = time.perf_counter()
        if i >= 2:
            tg.append((t1 - t0) * 1e3)
            tm.append((t2 - t1) * 1e3)
    res = {"gradient_call_ms": round(statistics.median(tg), 3), "motion_call_ms": round(statistics.median(tm), 3)}
    # the entries on their own, between device events
    stream = torch.cuda.current_stream(dev)
    a.set_stream(stream.cuda_stream)
    p0, p1 = pt.default_params(spp=2, spp_offset=0), pt.default_params(spp=2, spp_offset=2)
    prev, _ = a.render(cam, p0)
    lin, _ = a.render(cam, p1)
    feat = torch.from_numpy(a.render_features(cam, p1, 2)).to(dev)
    ids = torch.from_numpy(a.feature_ids(cam, p1)).to(dev)
    plane = torch.empty((S, S), dtype=torch.float32, device=dev)
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    g, dn0, tp = pt.default_gradient(), pt.default_denoise(iterations=0), pt.default_temporal()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    entry = [timed(lambda: check(lib().pt_temporal_gradient_device(a._h, C.byref(cam), C.byref(p0), k, P(prev), C.byref(g), 0.2, P(plane))))
             for k in range(9)][2:]
    ka = [timed(lambda: check(lib().pt_denoise_temporal_alpha_device(a._h, C.byref(cam), P(lin), P(feat), P(ids), P(plane), C.byref(dn0),
                                                                     C.byref(tp), P(out), P(rgba)))) for _ in range(9)][2:]
    km = [timed(lambda: check(lib().pt_denoise_temporal_motion_device(a._h, C.byref(cam), P(lin), P(feat), P(ids), C.byref(dn0), C.byref(tp),
                                                                      P(out), P(rgba)))) for _ in range(9)][2:]
    a.sync()
    res.update(gradient_entry_ms=round(statistics.median(entry), 4), alpha_kernel_ms=round(statistics.median(ka), 4),
               motion_kernel_ms=round(statistics.median(km), 4))
    a.close()
    b.close()
    return res


def quality(name, S):
    base = pt.builtin_scene(2)
    cam = pt.camera_new(width=S, height=S)
    ball = min((k for k, o in enumerate(base) if o.shape_tag == 0 and o.mat_tag != 1), key=lambda k: base[k].shape[3])
    N, change = (16, 1) if name == "moving" else (20, 8)

    def scene(i):
        objs = copy(base)
        if name == "moving":
            objs[ball].shape[0] += 0.02 * (i - N // 2)
        elif i >= change:
            for o in objs:
                if o.mat_tag == 1:
                    for k in range(3):
                        o.mat[k] *= 0.25
        return objs
    a, b, r = pt.Context(0), pt.Context(0), pt.Context(0)
    for c in (a, b, r):
        c.upload(scene(0))
    rel = {"gradient": [], "motion": []}
    raised = []
    ref = None
    for i in range(N):
        objs = scene(i)
        for c in (a, b):
            c.scene_update(objs)
        if ref is None or name == "moving" or i == change:
            r.scene_update(objs)
            ref = r.render(cam, pt.default_params(spp=1024, spp_offset=10 ** 6))[0].cpu().numpy().astype(np.float64)
        p = pt.default_params(spp=2, spp_offset=2 * i)
        fg = a.render_denoised_gradient(cam, p, 2)
        fm = b.render_denoised_motion(cam, p, 2)
        keep = fg[3][..., 3] == 0
        for key, f in (("gradient", fg), ("motion", fm)):
            rel[key].append(round(float(np.mean(((f[0].astype(np.float64) - ref) ** 2 / (ref ** 2 + 0.01))[keep])), 5))
        raised.append(round(float(np.mean(fg[5] > np.float32(0.2))), 4))
    res = {"frames": N, "change_at": change, "relmse_gradient": rel["gradient"], "relmse_motion": rel["motion"], "alpha_raised": raised}
    if name == "dimmed":
        for key in rel:
            steady = statistics.median(rel[key][change - 4:change])
            after = rel[key][change:]
            res["frames_to_steady_" + key] = next((k for k, v in enumerate(after) if v <= 1.25 * steady), None)
            res["steady_" + key] = steady
    for c in (a, b, r):
        c.close()
    return res


def orbit(k, S, step=0.006):
    """examples/gradient_frames.cpp --camera: the point of the circle of radius 2 whose half-angle tangent is step * k"""
    t = step * k
    q = 1.0 + t * t
    return pt.camera_look_at((2.0 * (2.0 * t) / q, 0.0, 2.0 * (1.0 - t * t) / q), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), S, S, 35.0)


def camera_cost(S, paths, rounds=7, per_round=3):
    objs = pt.builtin_scene(2)
    calls = {"existing": "render_denoised_gradient"}
    calls.update({p: "render_denoised_gradient_camera" for p in paths})
    ctx = {name: pt.Context(0) for name in calls}
    for c in ctx.values():
        c.upload(objs)
    times = {name: [] for name in calls}
    measured = {}
    frame = 0
    for r in range(rounds + 1):
        spent = {name: 0.0 for name in calls}
        for _ in range(per_round):
            p = pt.default_params(spp=2, spp_offset=2 * frame)
            for name, call in calls.items():
                cam = orbit(frame if name == "orbit" else 0, S)
                t0 = time.perf_counter()
                f = getattr(ctx[name], call)(cam, p, 2)
                spent[name] += time.perf_counter() - t0
                measured[name] = round(float(np.mean(~np.isnan(f[5]))), 4)
            frame += 1
        if r:
            for name in calls:
                times[name].append(spent[name] / per_round * 1e3)
    for c in ctx.values():
        c.close()
    return {name: {"frame_ms_median": round(statistics.median(t), 3), "frame_ms_min": round(min(t), 3), "frame_ms_max": round(max(t), 3),
                   "measured_last_frame": measured[name]} for name, t in times.items()}


def camera_quality(S, N=20, change=8):
    base = pt.builtin_scene(2)
    dim = copy(base)
    for o in dim:
        if o.mat_tag == 1:
            for k in range(3):
                o.mat[k] *= 0.25
    calls = {"motion": "render_denoised_motion", "gradient": "render_denoised_gradient", "gradient_camera": "render_denoised_gradient_camera"}
    ctx = {name: pt.Context(0) for name in calls}
    r = pt.Context(0)
    for c in list(ctx.values()) + [r]:
        c.upload(base)
    rel = {name: [] for name in calls}
    measured, raised = [], []
    for i in range(N):
        cam = orbit(i, S)
        if i == change:
            for c in list(ctx.values()) + [r]:
                c.scene_update(dim)
        ref = r.render(cam, pt.default_params(spp=1024, spp_offset=10 ** 6))[0].cpu().numpy().astype(np.float64)
        p = pt.default_params(spp=2, spp_offset=2 * i)
        for name, call in calls.items():
            f = getattr(ctx[name], call)(cam, p, 2)
            keep = f[3][..., 3] == 0
            rel[name].append(round(float(np.mean(((f[0].astype(np.float64) - ref) ** 2 / (ref ** 2 + 0.01))[keep])), 5))
            if name == "gradient":
                assert np.isnan(f[5]).all()                     # the camera moved: the existing entry measures nothing
            if name == "gradient_camera":
                measured.append(round(float(np.mean(~np.isnan(f[5]))), 4))
                raised.append(round(float(np.mean(f[5] > np.float32(0.2))), 4))
    res = {"frames": N, "change_at": change, "measured": measured, "alpha_raised": raised}
    for name in calls:
        steady = statistics.median(rel[name][change - 4:change])
        res["relmse_" + name] = rel[name]
        res["steady_" + name] = steady
        res["frames_to_steady_" + name] = next((k for k, v in enumerate(rel[name][change:]) if v <= 1.25 * steady), None)
    for c in list(ctx.values()) + [r]:
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--camera", action="store_true")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--paths", default="fixed,orbit")
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--sizes", default="128,1024")
    ap.add_argument("--quality-size", type=int, default=128)
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if args.camera:
        res = {"spp_per_frame": 2, "feature_samples": 2, "camera_cost": {f"c2_{args.size}": camera_cost(args.size, args.paths.split(","))}}
        if not args.skip_quality:
            res["camera_quality"] = camera_quality(args.quality_size)
        print(json.dumps(res))
        return
    res = {"spp_per_frame": 2, "feature_samples": 2, "cost": {}}
    for scene, label in ((2, "c2"), (1, "world_new")):
        for S in (int(s) for s in args.sizes.split(",")):
            res["cost"][f"{label}_{S}"] = cost(scene, S, args.frames)
    if not args.skip_quality:
        res["quality"] = {name: quality(name, args.quality_size) for name in ("moving", "dimmed")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
