"""Device-side BVH build (pt_scene_rebuild) against the host rebuild (pt_scene_update) and the refit (pt_scene_refit), on the job
of docs/EXPERIMENTS.md "Device-side refit": 10 000 spheres (builtin_scene(4, 10000)), accel = 1, every sphere moved a little per frame.

Prints one JSON line.  Every timing is taken --repeats times after one untimed round and reported as median, min and max:
  call_ms / call_and_first_render_ms   host time of the scene call alone and with the first 64 x 64 x 1 render behind it, for
                                       rebuild, update and refit, the three entries alternating frame by frame in one run
  rebuild_drain_ms                     host time from pt_scene_rebuild's return until the stream is idle (the build's kernels are
                                       the only work enqueued then: an upper bound of their GPU time)
  tree: render_morton_ms, render_sah_ms (GPU time of a 256 x 256 x 2 render over the device-built tree / over the host's SAH tree of
        the same pose) and the pt_scene_bvh_cost of both
  motion: 100 frames of motion, per frame one scene call and one 256 x 256 x 2 render: "refit" every frame, or a rebuild every k-th
          frame and a refit otherwise -- wall_ms of the 100 frames, and render_last_ms / cost_ratio_last of the tree at the end
--trace-loop N: nothing but N rebuilds of moving poses, for a kernel trace (the split into keys, sort, ids and refit)
--order median: the device builds are pt_scene_rebuild_ordered(PT_BVH_ORDER_MEDIAN) -- the drain, the motion table and the trace
          loop --, the alternating entries gain "rebuild_median" beside "rebuild" (Morton), and "tree" gains render_median_ms and
          cost_median beside the Morton and the SAH tree of the same pose

    python tools/rebuild_bench.py [--objects 10000] [--step 0.004] [--repeats 7] [--order morton|median]
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


def stat(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=10000)
    ap.add_argument("--step", type=float, default=0.004, help="largest move of a sphere per frame and axis")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace-loop", type=int, default=0)
    ap.add_argument("--order", choices=("morton", "median"), default="morton")
    args = ap.parse_args()
    median = args.order == "median"
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
    a.scene_rebuild_median = lambda objs: a.scene_rebuild(objs, order="median")
    rebuild = a.scene_rebuild_median if median else a.scene_rebuild      # the device build of --order

    if args.trace_loop:
        a.upload(base)
        for f in range(args.trace_loop):
            rebuild(pose(f))
        a.sync()
        a.close()
        b.close()
        return

    res = {"objects": n, "step": args.step, "repeats": args.repeats, "order": args.order}

    # ---- the scene call + the first render, the three entries alternating
    entries = (("rebuild_median",) if median else ()) + ("rebuild", "update", "refit")
    a.upload(base)
    a.render(small, p1)
    t = {e: ([], []) for e in entries}
    frame = 0
    for rep in range(args.repeats + 1):                  # (round 0 untimed: buffers grown, the topology cached)
        for entry in entries:                            # (refit comes behind update's render: it finds a tree)
            frame += 1
            objs = pose(frame)
            a.sync()
            t0 = time.perf_counter()
            getattr(a, "scene_" + entry)(objs)
            t1 = time.perf_counter()
            a.render(small, p1)
            a.sync()
            t2 = time.perf_counter()
            if rep:
                t[entry][0].append((t1 - t0) * 1e3)
                t[entry][1].append((t2 - t0) * 1e3)
    for entry in entries:
        res[entry] = {"call_ms": stat(t[entry][0]), "call_and_first_render_ms": stat(t[entry][1])}
    drain = []
    for _ in range(args.repeats):
        frame += 1
        rebuild(pose(frame))
        t1 = time.perf_counter()
        a.sync()
        drain.append((time.perf_counter() - t1) * 1e3)
    res["rebuild_drain_ms"] = stat(drain, 4)

    def render_ms(ctx):
        ts = []
        for _ in range(args.repeats + 1):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.render(big, p2)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts[1:]

    # ---- the Morton tree against the host's SAH tree of the same pose
    objs = pose(frame)
    a.scene_rebuild(objs)
    b.upload(objs)
    b.render(small, p1)
    res["tree"] = {"render_morton_ms": stat(render_ms(a), 4), "render_sah_ms": stat(render_ms(b), 4),
                   "cost_morton": a.bvh_cost()[0], "cost_sah": b.bvh_cost()[0]}
    if median:
        a.scene_rebuild_median(objs)
        res["tree"].update(render_median_ms=stat(render_ms(a), 4), cost_median=a.bvh_cost()[0])

    # ---- 100 frames of motion
    poses = [pose(f) for f in range(101)]
    res["motion"] = {}
    for every in (0, 10, 25, 50):
        a.upload(poses[0])
        rebuild(poses[0])
        a.render(big, p2)
        a.sync()
        t0 = time.perf_counter()
        for f in range(1, 101):
            (rebuild if every and f % every == 0 else a.scene_refit)(poses[f])
            a.render(big, p2)
        a.sync()
        wall = (time.perf_counter() - t0) * 1e3
        # the tree at the end, with the last rebuild's cost carried to this pose's grid by a fresh build of the same pose
        now = a.bvh_cost()[0]
        last = render_ms(a)
        rebuild(poses[100])
        res["motion"]["refit only" if not every else "rebuild every %d" % every] = {
            "wall_ms": round(wall, 2), "render_last_ms": stat(last, 4), "cost_ratio_last": round(now / a.bvh_cost()[0], 4)}
    a.close()
    b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
