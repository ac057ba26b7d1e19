"""The open-lens jobs of tests/test_gpu_lens_parity.py, shared with tests/test_oracle_lens.py, which checks on the CPU that the
f32 oracle stays within the FP32 bar of the f64 oracle on every one of them (the condition under which the fast-arithmetic GPU
cases can be asked the same).

A job is (scene, accel, integrator, lens, size, spp_offset, spp).  Routes: the LDS scan (scenes "diffuse" and "mirror", accel 0;
the two material sets k_paths is compiled for), the tiled scan ("tiled": 200 objects, accel 0) and the BVH (accel 1, any scene).
Every value of integrator, lens, size and spp_offset meets each of the three routes, the BVH meets each scene, and the wide lens
-- lens points outside the box, inside and behind objects -- meets every route.  37 x 23 x spp is no multiple of 64 or 256.
The two boxes are seen by the default camera; the camera of the sphere cloud stands inside it, (0, 0, -1.5), so that the wide
lens has spheres around, before and behind its points (from the default camera 7 of its 5106 lens rays hit anything).

A job that the reference itself does not pass cannot be asked of the GPU: ("diffuse", 0, BRDF, "wide", ODD, 5, 7) was replaced by
the same job at spp_offset 0, spp 6 -- at offset 5 one BRDF-only path that reaches the light in f64 and misses it in f32 moves the
mean of the 851 pixels by 6.4e-3 (bar: 1e-3), with 6, 7 or 8 samples alike."""
import numpy as np

SCENES = {"diffuse": (2, 0), "mirror": (1, 0), "tiled": (4, 200)}
LENSES = {"narrow": dict(aperture=0.2, focus_distance=2.0), "wide": dict(aperture=3.0, focus_distance=0.7)}
MIS, BRDF = 0, 1
BIG, ODD = (48, 40), (37, 23)

JOBS = [
    ("diffuse", 0, MIS, "narrow", BIG, 0, 6),
    ("diffuse", 0, BRDF, "wide", ODD, 0, 6),
    ("mirror", 0, MIS, "wide", BIG, 5, 8),
    ("mirror", 0, BRDF, "narrow", ODD, 0, 6),
    ("tiled", 0, MIS, "narrow", ODD, 0, 6),
    ("tiled", 0, BRDF, "wide", BIG, 5, 8),
    ("diffuse", 1, MIS, "wide", ODD, 5, 6),
    ("mirror", 1, BRDF, "narrow", BIG, 0, 8),
    ("tiled", 1, MIS, "narrow", BIG, 0, 7),
    ("tiled", 1, BRDF, "wide", ODD, 5, 6),
]


def job_id(job):
    scene, accel, integ, lens, (w, h), off, spp = job
    return f"{scene}-{'bvh' if accel else 'scan'}-{'brdf' if integ else 'mis'}-{lens}-{w}x{h}x{spp}+{off}"


def route(job):
    return "bvh" if job[1] else ("tiled" if job[0] == "tiled" else "lds")


def make(pt, job, **over):
    """-> (objs, cam, lens, params) of the job; over: further PtRenderParams fields (exact_math, bands, ...)"""
    scene, accel, integ, lens, (w, h), off, spp = job
    kw = dict(spp=spp, spp_offset=off, integrator=integ, accel=accel)
    kw.update(over)
    cam = pt.camera_new(origin=(0.0, 0.0, -1.5), width=w, height=h) if scene == "tiled" else pt.camera_new(width=w, height=h)
    return pt.builtin_scene(*SCENES[scene]), cam, pt.default_lens(**LENSES[lens]), pt.default_params(**kw)


def outside_bar(got, ref):
    """The FP32 bar as test_gpu_kernel_instances._within_bar states it -> (share of pixels with a channel outside
    |d| <= 1e-3 + 1e-2 |ref|, relative difference of the means)"""
    g = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    ok = (np.abs(g - r) <= 1e-3 + 1e-2 * np.abs(r)).all(-1)
    mean = abs(g.mean() - r.mean()) / r.mean() if r.mean() > 0 else 0.0
    return float(1.0 - ok.mean()), float(mean)


def within_bar(got, ref):
    """at least 99.5 % of pixels inside, the mean within 1e-3 relative"""
    share, mean = outside_bar(got, ref)
    assert 1.0 - share >= 0.995, f"{share:.4%} of {np.asarray(ref).size // 3} pixels outside the FP32 bar"
    assert mean <= 1e-3, f"mean off by {mean:.2e} relative"
