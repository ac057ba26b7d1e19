"""Device-side BVH refit (pt_scene_refit) against the host rebuild (pt_scene_update), on the job of docs/EXPERIMENTS.md
"Moving objects": 10 000 spheres (builtin_scene(4, 10000)), accel = 1, every sphere moved a little per frame.

Prints one JSON line, every figure a median of 5:
  *_call_ms, *_and_first_render_ms   host time of the scene call alone and with the first 64 x 64 x 1 render behind it, the two
                                     entries alternating frame by frame; update_and_first_render_spread_ms = max - min of its runs
  refit_drain_ms                     host time from pt_scene_refit's return until the stream is idle: the refit kernels are the
                                     only work enqueued then (an upper bound of their GPU time; their own time: a kernel trace)
  after_N: render_refit_ms, render_rebuilt_ms (GPU time of a 256 x 256 x 2 render over the tree refitted N times / over the tree
           rebuilt for the same pose), cost_ratio = cost_now / cost_at_build of the refitted tree

    python tools/refit_bench.py [--objects 10000] [--step 0.004]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtrace_amd as pt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=10000)
    ap.add_argument("--step", type=float, default=0.004, help="largest move of a sphere per frame and axis")
    args = ap.parse_args()
    base = pt.builtin_scene(4, args.objects)
    n = len(base)
    rng = np.random.default_rng(1)
    vel = rng.uniform(-args.step, args.step, (n, 3))

    def pose(frame):
        objs = (pt._lib.PtObject * n)(*base)
        for o, v in zip(objs, vel):
            for k in range(3):
                o.shape[k] += frame * v[k]
        return objs

    small, big = pt.camera_new(width=64, height=64), pt.camera_new(width=256, height=256)
    p1, p2 = pt.default_params(spp=1, accel=1), pt.default_params(spp=2, accel=1)
    a, b = pt.Context(0), pt.Context(0)
    res = {"objects": n, "step": args.step}

    # ---- the scene call + the first render, the two entries alternating
    a.upload(base)
    a.render(small, p1)
    a.scene_refit(pose(0))
    a.render(small, p1)                                  # (the scratch of the refit exists from here on)
    t = {"refit": ([], []), "update": ([], [])}
    frame = 0
    for _ in range(5):
        for entry in ("refit", "update"):                # (every entry ends in an accel = 1 render: the refit finds a tree)
            frame += 1
            objs = pose(frame)
            a.sync()
            t0 = time.perf_counter()
            (a.scene_refit if entry == "refit" else a.scene_update)(objs)
            t1 = time.perf_counter()
            a.render(small, p1)
            a.sync()
            t2 = time.perf_counter()
            t[entry][0].append((t1 - t0) * 1e3)
            t[entry][1].append((t2 - t0) * 1e3)
    for entry in ("refit", "update"):
        res[entry + "_call_ms"] = round(statistics.median(t[entry][0]), 3)
        res[entry + "_and_first_render_ms"] = round(statistics.median(t[entry][1]), 3)
        res[entry + "_and_first_render_spread_ms"] = round(max(t[entry][1]) - min(t[entry][1]), 3)
    drain = []
    for _ in range(5):
        frame += 1
        a.scene_refit(pose(frame))
        t1 = time.perf_counter()
        a.sync()
        drain.append((time.perf_counter() - t1) * 1e3)
    res["refit_drain_ms"] = round(statistics.median(drain), 4)

    # ---- quality of the refitted tree after 1, 10 and 100 frames of motion, against a rebuild for the same pose
    def render_ms(ctx):
        ts = []
        for _ in range(6):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.render(big, p2)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts[1:])

    a.upload(base)
    a.render(small, p1)
    done = 0
    for frames in (1, 10, 100):
        while done < frames:
            done += 1
            a.scene_refit(pose(done))
        b.upload(pose(done))
        now, at_build, refits = a.bvh_cost()
        assert refits == done
        res["after_%d" % frames] = {"render_refit_ms": round(render_ms(a), 4), "render_rebuilt_ms": round(render_ms(b), 4),
                                    "cost_ratio": round(now / at_build, 4)}
    a.close()
    b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
