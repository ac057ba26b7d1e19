#!/usr/bin/env python3
"""Adaptive sampling (pt_render_adaptive) on one GPU; prints one JSON line.
    python tools/adaptive_bench.py [--reps N] [--quick]

1. list_pass: a full-image pixel-list pass (the regenerating kernel's LIST instance) against the full-frame render, C2 and
   C1 at 1024^2 x 64 spp, in-order launches, alternating in the same process.  Both are isolated as differences of
   host-buffer calls, so that pass 0, the PCIe copies and the call overhead cancel:
       full-frame 64 spp = t(pt_render_host, spp 66) - t(pt_render_host, spp 2)
       list pass  64 spp = t(pt_render_adaptive, spp_min 2, spp_step 64, spp_max 66, rel_tol 0) - t(pt_render_host, spp 2)
   (the list pass's figure also carries one k_adaptive_select and its 4-byte read-back, and the adaptive call copies two
   more output planes back).  The same differences of the path kernels' own time (PtRenderParams.profile = 1: HIP events
   around every path-kernel launch, PtStats.bounce_kernel_ms) compare the kernels alone.
2. world: World::new() 400^2, spp_max 3000, spp_min = spp_step = 64, at two tolerances: wall time, sum of spp, the spp
   histogram, passes, against the uniform 3000 spp render (pt_render_host) measured in the same process; a profiled run
   gives the path kernels' share, the rest divided by the passes is the fixed cost of a pass (resolve, select, read-back,
   host round trip, launch)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pathtrace_amd as pt  # noqa: E402
from pathtrace_amd._lib import check, lib  # noqa: E402


def render_host(ctx, cam, prm, lin, rgba):
    check(lib().pt_render_host(ctx._h, C.byref(cam), C.byref(prm), lin.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)))


def timed(fn, reps):
    fn()                                  # warm-up (allocations, occupancy queries)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def list_pass(ctx, scene, reps, size):
    ctx.upload(pt.builtin_scene(scene))
    ctx.set_tuning(in_order=1)
    cam = pt.camera_new(width=size, height=size)
    lin = np.empty((size, size, 3), np.float32)
    rgba = np.empty((size, size, 4), np.uint8)
    p2, p66 = pt.default_params(spp=2), pt.default_params(spp=66)
    t2, t66, tad = [], [], []
    for _ in range(reps):                 # alternating, so that drifts of clock or temperature hit all three alike
        t2 += timed(lambda: render_host(ctx, cam, p2, lin, rgba), 1)
        t66 += timed(lambda: render_host(ctx, cam, p66, lin, rgba), 1)
        tad += timed(lambda: ctx.render_adaptive(cam, p66, spp_min=2, spp_step=64, rel_tol=0.0), 1)
    k2, k66, kad = [], [], []
    q2, q66 = pt.default_params(spp=2, profile=1), pt.default_params(spp=66, profile=1)
    for _ in range(reps):
        render_host(ctx, cam, q2, lin, rgba); k2.append(ctx.stats().bounce_kernel_ms)
        render_host(ctx, cam, q66, lin, rgba); k66.append(ctx.stats().bounce_kernel_ms)
        ctx.render_adaptive(cam, q66, spp_min=2, spp_step=64, rel_tol=0.0); kad.append(ctx.stats().bounce_kernel_ms)
    ctx.set_tuning()
    kfull = statistics.median(k66) - statistics.median(k2)
    klist = statistics.median(kad) - statistics.median(k2)
    m2, m66, mad = statistics.median(t2), statistics.median(t66), statistics.median(tad)
    paths = size * size * 64
    full, lst = m66 - m2, mad - m2
    return {"scene": f"C{scene}", "size": size, "spp": 64, "ms_host_spp2": round(m2, 3), "ms_host_spp66": round(m66, 3),
            "ms_adaptive_2_plus_64": round(mad, 3), "ms_full_frame_64": round(full, 3), "ms_list_pass_64": round(lst, 3),
            "msamples_s_full_frame": round(paths / full / 1e3, 1), "msamples_s_list_pass": round(paths / lst / 1e3, 1),
            "list_over_full": round(full / lst, 3), "kernel_ms_full_frame_64": round(kfull, 3), "kernel_ms_list_pass_64": round(klist, 3),
            "kernel_list_over_full": round(kfull / klist, 3)}


def world(ctx, reps, tols, size, spp_max):
    ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=size, height=size)
    prm = pt.default_params(spp=spp_max)
    lin = np.empty((size, size, 3), np.float32)
    rgba = np.empty((size, size, 4), np.uint8)
    uni = timed(lambda: render_host(ctx, cam, prm, lin, rgba), reps)
    out = {"size": size, "spp_max": spp_max, "spp_min": 64, "spp_step": 64, "ms_uniform": round(statistics.median(uni), 3), "runs": []}
    for tol in tols:
        res = {}
        def run():
            res["r"] = ctx.render_adaptive(cam, prm, spp_min=64, spp_step=64, rel_tol=tol, abs_floor=1e-3)
        ms = timed(run, reps)
        _, _, spp, err = res["r"]
        st = ctx.stats()
        ctx.render_adaptive(cam, pt.default_params(spp=spp_max, profile=1), spp_min=64, spp_step=64, rel_tol=tol, abs_floor=1e-3)
        kms = ctx.stats().bounce_kernel_ms
        passes = 1 + -(-(int(spp.max()) - 64) // 64)
        vals, cnt = np.unique(spp, return_counts=True)
        out["runs"].append({"rel_tol": tol, "ms": round(statistics.median(ms), 3), "ms_all": [round(x, 3) for x in ms],
                            "sum_spp": int(spp.sum(dtype=np.uint64)), "uniform_spp": size * size * spp_max,
                            "samples_counted": int(st.samples), "passes": passes,
                            "kernel_ms": round(kms, 3), "fixed_ms_per_pass": round((statistics.median(ms) - kms) / passes, 3),
                            "bounce_launches": int(st.bounce_launches), "spp_hist": {int(v): int(c) for v, c in zip(vals, cnt)},
                            "rel_err_median": float(np.median(err)), "rel_err_p99": float(np.quantile(err, 0.99))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of the tool itself)")
    a = ap.parse_args()
    ctx = pt.Context(0)
    size, wsize, smax = (256, 128, 512) if a.quick else (1024, 400, 3000)
    rec = {"tool": "adaptive_bench", "list_pass": [list_pass(ctx, s, a.reps, size) for s in (2, 1)],
           "world": world(ctx, a.reps, (0.02, 0.05), wsize, smax)}
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
