"""The irradiance volume (pt_probe_grid_bake_device, pt_probe_shade_device, pt_render_probe_lit_device) on builtin
scene 2, one JSON line:
  shade        k_probe_shade at --size^2 against grids of 4^3 and 16^3 probes, both weight modes.  Per form `--runs` timings between
               device events, each over `--reps` launches enqueued back to back (us per launch: all of them, the median, the spread
               max - min), the forms alternating inside every run.
  frame        pt_render_probe_lit_device (1 feature sample) beside pt_render_device at 1 and 16 spp, the same way (ms).
  quality      relMSE = mean((a - ref)^2 / (ref^2 + 1e-2)) at 256^2 against a --ref-spp PT_INTEGRATOR_BRDF_ONLY render: the probe-lit
               frame (8^3 probes, 256 rays x 16 spp each, emitter and miss pixels from the 1-spp render), and the plain renders of
               1, 2, 4, 8 and 16 spp with their times, of which the cheapest is already dearer than the probe-lit frame.
The probe-lit frame is biased by construction: light leaks through walls (no per-probe visibility) and mirrors are shaded as
diffuse surfaces of their colour."""
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


def box_grid(n):
    """n^3 probes in the box of builtin scene 2, [-1, 1]^2 x [-3, -1], a tenth away from the walls"""
    return pt.probe_grid((-0.9, -0.9, -2.9), (1.8 / (n - 1),) * 3, (n, n, n))


def timed(ctx, forms, runs, reps):
    times = {k: [] for k in forms}
    for run in range(runs + 1):                                   # the first round warms up
        for name, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            ctx.sync()
            e1.synchronize()
            if run:
                times[name].append(e0.elapsed_time(e1) / reps)
    return times


def summary(t, scale, digits):
    return {"all": [round(v * scale, digits) for v in t], "median": round(statistics.median(t) * scale, digits),
            "spread": round((max(t) - min(t)) * scale, digits)}


def rel_mse(a, ref):
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    return float(np.mean((a - ref) ** 2 / (ref ** 2 + 1e-2)))


def visibility(a):
    """--visibility, one JSON line: k_probe_moments for 16^3 probes x 256 rays at T = 8 and 16 (us); k_probe_shade_vis
    at --size^2 beside k_probe_shade FACING on the same 16^3 grid, the forms alternating (us); the probe-lit frame with and without
    the term (ms).  The leak numbers are those tests/test_gpu_probe_vis.py prints (pytest -s)."""
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(2))
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = pt._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    S = a.size
    cam = pt.camera_new(width=S, height=S)
    prm1 = pt.default_params(spp=1)
    feat = torch.from_numpy(ctx.render_features(cam, prm1, 1)).to(dev)
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    g = box_grid(16)
    sh = ctx.probe_grid_bake(g, 64, prm1)
    dist = ctx.probe_distances(pt.probe_grid_positions(g), 256, prm1)
    sp = pt.default_probe_shade(normal_bias=0.02, weight=1)
    vis = {T: pt.default_probe_visibility(g, resolution=T) for T in (8, 16)}
    maps = {T: ctx.probe_moments(dist, vis[T]) for T in (8, 16)}
    out = {"size": S, "runs": a.runs, "reps": a.reps}
    moments = {f"T={T}": lambda T=T: pt._lib.check(L.pt_probe_moments_device(ctx._h, p(dist), 4096, 256, C.byref(vis[T]), p(maps[T]))) for T in (8, 16)}
    out["moments_us"] = {k: summary(t, 1e3, 2) for k, t in timed(ctx, moments, a.runs, a.reps).items()}
    shade = {"facing": lambda: pt._lib.check(L.pt_probe_shade_device(ctx._h, C.byref(cam), C.byref(g), p(sh), p(feat), None, C.byref(sp), p(lin), p(rgba)))}
    frame = {"probe_lit": lambda: pt._lib.check(L.pt_render_probe_lit_device(ctx._h, C.byref(cam), C.byref(prm1), 1, C.byref(g), p(sh), None, C.byref(sp),
                                                                             p(lin), p(rgba)))}
    for T in (8, 16):
        shade[f"visibility T={T}"] = lambda T=T: pt._lib.check(L.pt_probe_shade_visibility_device(
            ctx._h, C.byref(cam), C.byref(g), p(sh), p(maps[T]), C.byref(vis[T]), p(feat), None, C.byref(sp), p(lin), p(rgba)))
        frame[f"probe_lit_visibility T={T}"] = lambda T=T: pt._lib.check(L.pt_render_probe_lit_visibility_device(
            ctx._h, C.byref(cam), C.byref(prm1), 1, C.byref(g), p(sh), p(maps[T]), C.byref(vis[T]), None, C.byref(sp), p(lin), p(rgba)))
    out["shade_us"] = {k: summary(t, 1e3, 2) for k, t in timed(ctx, shade, a.runs, a.reps).items()}
    out["frame_ms"] = {k: summary(t, 1.0, 4) for k, t in timed(ctx, frame, a.runs, 4).items()}
    print(json.dumps(out))
    ctx.close()


def update(a):
    """--update, one JSON line, builtin scene 2, 16^3 probes, T = 8: k_probe_update on 4096 slots x 64 rays beside
    k_probe_sh + k_probe_moments on the same planes (us); one stride-8 update of 64 rays end to end beside the full bake and
    visibility pass at 256 rays (ms); the probe-lit frame with the visibility term alone and behind a stride-8 update (ms)."""
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(2))
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = pt._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    S = a.size
    cam = pt.camera_new(width=S, height=S)
    prm1 = pt.default_params(spp=1)
    g = box_grid(16)
    P, T = 4096, 8
    vis = pt.default_probe_visibility(g, resolution=T)
    sp = pt.default_probe_shade(normal_bias=0.02, weight=1)
    rad, sh = ctx.bake_probes(pt.probe_grid_positions(g), 64, prm1)
    dist = ctx.probe_distances(pt.probe_grid_positions(g), 64, prm1)
    maps = ctx.probe_moments(dist, vis)
    age = torch.full((P,), 16, dtype=torch.int32, device=dev)
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    sh2, maps2 = sh.clone(), maps.clone()
    all_slots = pt.default_probe_update(1, 1)
    stride8 = pt.default_probe_update(1, 8)
    out = {"size": S, "runs": a.runs, "reps": a.reps}

    def separate():
        pt._lib.check(L.pt_sh_project_device(ctx._h, P, 64, p(rad), p(sh2)))
        pt._lib.check(L.pt_probe_moments_device(ctx._h, p(dist), P, 64, C.byref(vis), p(maps2)))

    kernels = {"k_probe_update": lambda: pt._lib.check(L.pt_probe_blend_device(ctx._h, P, C.byref(all_slots), C.byref(vis), p(rad), p(dist), p(sh), p(maps),
                                                                               p(age))),
               "k_probe_update, no maps": lambda: pt._lib.check(L.pt_probe_blend_device(ctx._h, P, C.byref(all_slots), None, p(rad), None, p(sh), None, p(age))),
               "k_probe_sh + k_probe_moments": separate,
               "k_probe_sh": lambda: pt._lib.check(L.pt_sh_project_device(ctx._h, P, 64, p(rad), p(sh2)))}
    out["kernels_us"] = {k: summary(t, 1e3, 2) for k, t in timed(ctx, kernels, a.runs, a.reps).items()}

    def full():
        pt._lib.check(L.pt_probe_grid_bake_device(ctx._h, C.byref(g), 256, C.byref(prm1), p(sh2)))
        pt._lib.check(L.pt_probe_grid_visibility_device(ctx._h, C.byref(g), 256, C.byref(prm1), C.byref(vis), p(maps2)))

    upd_call = lambda: pt._lib.check(L.pt_probe_grid_update_device(ctx._h, C.byref(g), C.byref(prm1), C.byref(vis), C.byref(stride8), p(sh), p(maps), p(age)))
    frame_call = lambda: pt._lib.check(L.pt_render_probe_lit_visibility_device(ctx._h, C.byref(cam), C.byref(prm1), 1, C.byref(g), p(sh), p(maps),
                                                                               C.byref(vis), None, C.byref(sp), p(lin), p(rgba)))
    whole = {"update stride 8, 64 rays": upd_call, "bake + visibility, 256 rays": full, "probe_lit_visibility": frame_call,
             "update stride 8 + probe_lit_visibility": lambda: (upd_call(), frame_call())}
    out["calls_ms"] = {k: summary(t, 1.0, 4) for k, t in timed(ctx, whole, a.runs, 4).items()}
    print(json.dumps(out))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--visibility", action="store_true", help="the probe-visibility kernels and frame instead (DESIGN.md 5t)")
    ap.add_argument("--update", action="store_true", help="the update kernel and calls instead (DESIGN.md 5u)")
    a = ap.parse_args()
    if a.visibility:
        return visibility(a)
    if a.update:
        return update(a)
    ctx = pt.Context(0)
    ctx.upload(pt.builtin_scene(2))
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = pt._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    S = a.size
    cam = pt.camera_new(width=S, height=S)
    feat = torch.from_numpy(ctx.render_features(cam, pt.default_params(spp=1), 1)).to(dev)
    lin = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    rgba = torch.empty((S, S, 4), dtype=torch.uint8, device=dev)
    out = {"size": S, "runs": a.runs, "reps": a.reps}
    # ---- the kernel
    forms = {}
    keep = []
    for n in (4, 16):
        g = box_grid(n)
        sh = ctx.probe_grid_bake(g, 64, pt.default_params(spp=1))
        keep.append((g, sh))
        for wname, w in (("trilinear", 0), ("facing", 1)):
            sp = pt.default_probe_shade(normal_bias=0.02, weight=w)
            keep.append(sp)
            forms[f"{n}^3 {wname}"] = lambda g=g, sh=sh, sp=sp: pt._lib.check(
                L.pt_probe_shade_device(ctx._h, C.byref(cam), C.byref(g), p(sh), p(feat), None, C.byref(sp), p(lin), p(rgba)))
    out["shade_us"] = {k: summary(t, 1e3, 2) for k, t in timed(ctx, forms, a.runs, a.reps).items()}
    # ---- the frame
    g8 = box_grid(8)
    sh8 = ctx.probe_grid_bake(g8, 256, pt.default_params(spp=16, integrator=1))
    sp = pt.default_probe_shade(normal_bias=0.02, weight=1)
    prm1, prm16 = pt.default_params(spp=1), pt.default_params(spp=16)
    frame = {
        "probe_lit": lambda: pt._lib.check(L.pt_render_probe_lit_device(ctx._h, C.byref(cam), C.byref(prm1), 1, C.byref(g8), p(sh8), None, C.byref(sp),
                                                                        p(lin), p(rgba))),
        "render_1spp": lambda: pt._lib.check(L.pt_render_device(ctx._h, C.byref(cam), C.byref(prm1), p(lin), p(rgba))),
        "render_16spp": lambda: pt._lib.check(L.pt_render_device(ctx._h, C.byref(cam), C.byref(prm16), p(lin), p(rgba))),
    }
    out["frame_ms"] = {k: summary(t, 1.0, 4) for k, t in timed(ctx, frame, a.runs, 4).items()}
    # ---- the quality at 256^2
    Q = 256
    camq = pt.camera_new(width=Q, height=Q)
    ref = ctx.render(camq, pt.default_params(spp=a.ref_spp, integrator=1), want_rgba=False)[0].cpu().numpy()
    quality = {"ref_spp": a.ref_spp}
    linq = torch.empty((Q, Q, 3), dtype=torch.float32, device=dev)
    plain = {}
    for spp in (1, 2, 4, 8, 16):
        prm = pt.default_params(spp=spp, integrator=1, spp_offset=a.ref_spp)
        t = timed(ctx, {"r": lambda prm=prm: pt._lib.check(L.pt_render_device(ctx._h, C.byref(camq), C.byref(prm), p(linq), None))}, a.runs, 4)["r"]
        plain[spp] = {"rel_mse": rel_mse(linq.cpu().numpy(), ref), "ms": round(statistics.median(t), 4)}
    quality["plain"] = plain
    fb = ctx.render(camq, pt.default_params(spp=1, integrator=1, spp_offset=a.ref_spp), want_rgba=False)[0]
    call = lambda: pt._lib.check(L.pt_render_probe_lit_device(ctx._h, C.byref(camq), C.byref(prm1), 1, C.byref(g8), p(sh8), p(fb), C.byref(sp), p(linq), None))
    t = timed(ctx, {"p": call}, a.runs, 4)["p"]
    quality["probe_lit"] = {"rel_mse": rel_mse(linq.cpu().numpy(), ref), "ms": round(statistics.median(t), 4), "grid": "8^3", "rays_per_probe": 256,
                            "bake_spp": 16}
    out["quality_256"] = quality
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
