"""Thin-lens render (pt_render_lens_device) beside the pinhole render of the same job, alternating in one process:
C2 at 1024^2 x 16 spp by default, aperture 0.2.  Per form the wall time of `--runs` renders between device events (ms, all of
them and the median): the pinhole render in the default (regenerating) form, the pinhole render in the queue form
(level0_form = 1) and the lens render, which takes the queue form's kernels.  k_source_paths<LensSource>'s own time: run this tool under a
kernel trace.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pathtrace_amd as pt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=2)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--aperture", type=float, default=0.2)
    ap.add_argument("--focus", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--max-paths", type=int, default=0)
    a = ap.parse_args()
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(a.scene))
    cam = pt.camera_new(width=a.size, height=a.size)
    prm = pt.default_params(spp=a.spp, max_paths_in_flight=a.max_paths)
    lens = pt.default_lens(aperture=a.aperture, focus_distance=a.focus)
    dev = torch.device("cuda", 0)
    lin = torch.empty((a.size, a.size, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = pt._lib.lib()
    import ctypes as C

    def pinhole():
        ctx.render_into(cam, prm, lin.data_ptr(), rgba.data_ptr())

    def through_lens():
        pt._lib.check(L.pt_render_lens_device(ctx._h, C.byref(cam), C.byref(lens), C.byref(prm), C.c_void_p(lin.data_ptr()), C.c_void_p(rgba.data_ptr())))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ctx.sync()
        e1.synchronize()
        return e0.elapsed_time(e1)

    forms = {"pinhole_ms": (0, pinhole), "pinhole_queue_form_ms": (1, pinhole), "lens_ms": (0, through_lens)}
    times = {k: [] for k in forms}
    for r in range(a.runs + 1):              # the first round warms up
        for name, (form, fn) in forms.items():
            ctx.set_tuning(level0_form=form)
            t = timed(fn)
            if r:
                times[name].append(round(t, 4))
    out = {"scene": a.scene, "size": a.size, "spp": a.spp, "aperture": a.aperture, "focus": a.focus, "runs": a.runs}
    for k, v in times.items():
        out[k] = v
        out[k.replace("_ms", "_median_ms")] = round(statistics.median(v), 4)
    out["lens_over_queue_form"] = round(out["lens_median_ms"] / out["pinhole_queue_form_median_ms"], 3)
    out["lens_gsamples_per_s"] = round(a.size * a.size * a.spp / out["lens_median_ms"] / 1e6, 3)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
