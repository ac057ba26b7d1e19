"""Light baking (pt_bake_lightmap_device, pt_bake_probes_device, pt_sh_project_device) beside pt_render_rays_device
fed the bake's own rays, alternating in one process: a 256^2 x 64 spp lightmap of the floor of World::new() (builtin scene 1) and
4096 probes x 256 rays in its box by default.  Per form the wall time of `--runs` calls between device events (ms, all of them,
the median and the spread max - min).  A bake enqueues the path launches of the render of its rays; what differs is the fill
(k_source_paths<BakeSource> computes the rays, k_source_paths<CallerSource> reads them) and what follows the resolve (k_bake_mask; k_probe_sh, which is also
timed alone through pt_sh_project_device).  The kernels' own durations: run this tool under a kernel trace.  One JSON line."""
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


def all_xys(W, H, s):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, s)], axis=1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=1)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(a.scene))
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = pt._lib.lib()
    N, P, R = a.size, a.probes, a.rays
    # the floor of the box: y = -1, x in [-1, 1], z in [-3, -1], normal +y
    g = (np.arange(N) + 0.5) / N * 2.0 - 1.0
    tex = np.zeros((N, N, 6), dtype=np.float32)
    tex[..., 0], tex[..., 1], tex[..., 2], tex[..., 4] = g[None, :], -1.0, g[:, None] - 2.0, 1.0
    d_tex = torch.from_numpy(tex).to(dev)
    rng = np.random.default_rng(1)
    pos = (rng.uniform(-0.9, 0.9, (P, 3)) + np.array([0.0, 0.0, -2.0])).astype(np.float32)
    d_pos = torch.from_numpy(pos).to(dev)
    prm_map = pt.default_params(spp=a.spp)
    prm_probe = pt.default_params(spp=1)
    lin = torch.empty((N, N, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((N, N, 4), dtype=torch.uint8, device=dev)
    rad = torch.empty((P, R, 3), dtype=torch.float32, device=dev)
    sh = torch.empty((P, 9, 3), dtype=torch.float32, device=dev)
    # the bakes' own rays as a caller's planes, a sample at a time through the debug entry
    map_rays = torch.empty((a.spp, N, N, 6), dtype=torch.float32, device=dev)
    for s in range(a.spp):
        map_rays[s] = torch.from_numpy(ctx.bake_rays("texels", tex, all_xys(N, N, s)).reshape(N, N, 6)).to(dev)
    probe_rays = torch.from_numpy(ctx.bake_rays("probes", (pos, R), all_xys(R, P, 0)).reshape(1, P, R, 6)).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    forms = {
        "bake_lightmap": lambda: pt._lib.check(L.pt_bake_lightmap_device(ctx._h, N, N, p(d_tex), C.byref(prm_map), p(lin), p(rgba))),
        "render_rays_lightmap": lambda: pt._lib.check(L.pt_render_rays_device(ctx._h, N, N, C.byref(prm_map), p(map_rays), None, p(lin), p(rgba))),
        "bake_probes": lambda: pt._lib.check(L.pt_bake_probes_device(ctx._h, p(d_pos), P, R, C.byref(prm_probe), p(rad), p(sh))),
        "render_rays_probes": lambda: pt._lib.check(L.pt_render_rays_device(ctx._h, R, P, C.byref(prm_probe), p(probe_rays), None, p(rad), None)),
        "sh_project": lambda: pt._lib.check(L.pt_sh_project_device(ctx._h, P, R, p(rad), p(sh))),
    }
    times = {k: [] for k in forms}
    for run in range(a.runs + 1):                                 # the first round warms up
        for name, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            ctx.sync()
            e1.synchronize()
            if run:
                times[name].append(e0.elapsed_time(e1))
    out = {"scene": a.scene, "lightmap": [N, N, a.spp], "probes": [P, R], "runs": a.runs}
    for name, t in times.items():
        out[name] = {"ms": [round(v, 4) for v in t], "median_ms": round(statistics.median(t), 4), "spread_ms": round(max(t) - min(t), 4)}
    out["lightmap_minus_render_rays_ms"] = round(out["bake_lightmap"]["median_ms"] - out["render_rays_lightmap"]["median_ms"], 4)
    out["probes_minus_render_rays_ms"] = round(out["bake_probes"]["median_ms"] - out["render_rays_probes"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
