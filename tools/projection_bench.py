"""Projection renders and films from caller rays (pt_render_projection_device, pt_render_rays_device) beside the
lens render at aperture 0, alternating in one process: C2 at 1024^2 x 16 spp by default.  Per form the wall time of `--runs`
renders between device events (ms, all of them, the median and the spread max - min): the lens render, the projection render
of every kind, and the render of caller rays (the pinhole's own, written once by the debug entry in chunks).  All of them
enqueue the same path launches; what differs is the launch that writes the path states.  The fill kernels' own times
(k_source_paths<LensSource>, <ProjectionSource>, <CallerSource>): run this tool under a kernel trace; `bytes` below is what each of them moves
per render (four 16-byte state planes written per path; the caller-ray instance also reads 24 bytes per path), for bytes / s against the
HBM peak.  One JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=2)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--fov", type=float, default=180.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-paths", type=int, default=0)
    a = ap.parse_args()
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(a.scene))
    cam = pt.camera_new(width=a.size, height=a.size)
    prm = pt.default_params(spp=a.spp, max_paths_in_flight=a.max_paths)
    lens = pt.default_lens()
    dev = torch.device("cuda", 0)
    lin = torch.empty((a.size, a.size, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = pt._lib.lib()
    out_ptrs = (C.c_void_p(lin.data_ptr()), C.c_void_p(rgba.data_ptr()))
    # the pinhole's own rays as the caller's planes, one image row of all samples at a time through the debug entry
    rays = torch.empty((a.spp, a.size, a.size, 6), dtype=torch.float32, device=dev)
    xs, ss = np.meshgrid(np.arange(a.size), np.arange(a.spp), indexing="xy")
    for y in range(a.size):
        xys = np.stack([xs.ravel(), np.full(xs.size, y), ss.ravel()], axis=1).astype(np.uint32)
        rays[:, y] = torch.from_numpy(ctx.debug_camera_rays(cam, xys)[:, :6].reshape(a.spp, a.size, 6)).to(dev)

    def through_lens():
        pt._lib.check(L.pt_render_lens_device(ctx._h, C.byref(cam), C.byref(lens), C.byref(prm), *out_ptrs))

    def projection(kind):
        proj = pt.default_projection(kind=kind, fov_degrees=a.fov)
        return lambda: pt._lib.check(L.pt_render_projection_device(ctx._h, C.byref(cam), C.byref(proj), C.byref(prm), *out_ptrs))

    def caller_rays():
        pt._lib.check(L.pt_render_rays_device(ctx._h, a.size, a.size, C.byref(prm), C.c_void_p(rays.data_ptr()), None, *out_ptrs))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ctx.sync()
        e1.synchronize()
        return e0.elapsed_time(e1)

    forms = {"lens_aperture0_ms": through_lens, "perspective_ms": projection("perspective"), "orthographic_ms": projection("orthographic"),
             "fisheye_ms": projection("fisheye"), "equirect_ms": projection("equirect"), "caller_rays_ms": caller_rays}
    times = {k: [] for k in forms}
    for r in range(a.runs + 1):              # the first round warms up
        for name, fn in forms.items():
            t = timed(fn)
            if r:
                times[name].append(round(t, 4))
    paths = a.size * a.size * a.spp
    out = {"scene": a.scene, "size": a.size, "spp": a.spp, "fov": a.fov, "runs": a.runs,
           "fill_bytes": {"k_source_paths<LensSource>": 64 * paths, "k_source_paths<ProjectionSource>": 64 * paths, "k_source_paths<CallerSource>": 88 * paths}}
    for k, v in times.items():
        out[k] = v
        out[k.replace("_ms", "_median_ms")] = round(statistics.median(v), 4)
        out[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
    out["perspective_minus_lens_ms"] = round(out["perspective_median_ms"] - out["lens_aperture0_median_ms"], 4)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
